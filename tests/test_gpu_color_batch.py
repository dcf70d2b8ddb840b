"""Textured renders of several views in one launch sequence: SDFRenderer_color.render_batch / relight, decode_color_batch
(distr_color_*_multi, distr_color_stage_*).

The contracts are byte equalities wherever the arithmetic is the same -- a segment against the single-code call, a view of a batch
against its own B = 1 call, a relit frame against the lit render -- so the pins of the single paths (oracle, goldens G10 / G13 / G26) carry
over; against the composed single-view path (`render`, whose points are formed by torch in another f32 order) the bars are the existing
tests' own. Image size 48 x 45: 2160 pixels are two compaction blocks of 2048 per view; fixture F1, 30 march steps; three cameras whose
valid-pixel counts are neither 0 nor multiples of 64, and one that looks past the shape (count 0).
"""
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

SIZES = [1, 64, 65, 0, 130, 63]
H, W = 48, 45
CS = 32                                           # colour code length of the batch tests (G26's)
CAMS = [(30.0, 20.0, 1.6, 10.0), (-75.0, -35.0, 1.9, 0.0), (160.0, 5.0, 1.45, -20.0)]      # azimuth, elevation, distance, roll
LIGHTS = np.array([[1.5, 2.0, -1.0], [-2.0, 0.5, 2.5], [0.3, -2.5, -2.0]], dtype=np.float32)
ENERGIES = np.array([0.9, 0.6, 0.4], dtype=np.float32)


def _module(Ws, bs, latent, dims, last):
    import torch
    from core.graph.deep_sdf_decoder import Decoder
    d = Decoder(latent, dims, last_dim=last, norm_layers=(), latent_in=[4])
    d.load_state_dict({('lin%d.%s' % (l, n)): torch.from_numpy(a) for l, (Wl, bl) in enumerate(zip(Ws, bs)) for n, a in (('weight', Wl), ('bias', bl))})
    return d.cuda().eval()


def _decoders(fixture_decoder, cs):
    from distr import fixture
    Ws, bs, latent = fixture_decoder
    Wc, bc, code = fixture.make_color_decoder_weights(color_size=cs)
    dims_c = [512] * 8
    dims_c[3] += cs
    return _module(Ws, bs, 256, [512] * 8, 1), _module(Wc, bc, 256 + cs, dims_c, 3), latent, code


def _eq(a, b):
    return a.shape == b.shape and a.detach().cpu().numpy().tobytes() == b.detach().cpu().numpy().tobytes()


def _segments(sizes):
    at = 0
    for s, n in enumerate(sizes):
        yield s, at, at + n
        at += n


# ------------------------------------------------------------------------------------------ 1. colour on a segmented point list
@pytest.fixture(scope='module')
def color_case(fixture_decoder):
    """(colour decoder module, colour codes (6, cs), shape codes (6, 256), points, upstream gradient): made once, never modified."""
    import torch
    _, dec_c, latent, code = _decoders(fixture_decoder, CS)
    rs = np.random.RandomState(77)
    sc = (latent + 0.3 * np.abs(latent).max() * rs.standard_normal((len(SIZES), 256))).astype(np.float32)
    cc = (code + 0.3 * np.abs(code).max() * rs.standard_normal((len(SIZES), CS))).astype(np.float32)
    pts = ((rs.rand(sum(SIZES), 3) - 0.5) * 1.6).astype(np.float32)
    w = rs.standard_normal((sum(SIZES), 3)).astype(np.float32)
    return dec_c, torch.from_numpy(cc).cuda(), torch.from_numpy(sc).cuda(), torch.from_numpy(pts).cuda(), torch.from_numpy(w).cuda()


def _single(dec_c, cc, sc, pts, w):
    """decode_color of one segment with its gradients: (rgb, g_color_code, g_shape_code, g_points)."""
    from core.utils.decoder_utils import decode_color
    c1, s1, x1 = cc.clone().requires_grad_(True), sc.clone().requires_grad_(True), pts.clone().requires_grad_(True)
    y = decode_color(dec_c, c1, s1, x1)
    (y * w).sum().backward()
    return y.detach(), c1.grad, s1.grad, x1.grad


def test_segmented_decode_equals_single_calls(color_case):
    import torch
    from core.utils.decoder_utils import decode_color_batch
    dec_c, cc, sc, pts, w = color_case
    outs = []
    for _ in range(2):                                              # the same bytes on every run
        c, s, x = cc.clone().requires_grad_(True), sc.clone().requires_grad_(True), pts.clone().requires_grad_(True)
        y = decode_color_batch(dec_c, c, s, x, counts=SIZES)
        (y * w).sum().backward()
        outs.append((y.detach(), c.grad, s.grad, x.grad))
    assert all(_eq(a, b) for a, b in zip(*outs))
    y, g_c, g_s, g_x = outs[0]
    assert y.shape == (sum(SIZES), 3) and g_c.shape == cc.shape and g_s.shape == sc.shape and g_x.shape == pts.shape
    for s, a, b in _segments(SIZES):
        if a == b:
            assert not g_c[s].any() and not g_s[s].any(), 'the empty segment has a code gradient'
            continue
        y1, c1, s1, x1 = _single(dec_c, cc[s:s + 1], sc[s:s + 1], pts[a:b], w[a:b])
        assert _eq(y[a:b], y1) and _eq(g_x[a:b], x1) and _eq(g_c[s:s + 1], c1) and _eq(g_s[s:s + 1], s1), s
    assert y.abs().max() > 0 and g_x.abs().max() > 0 and g_c.abs().max() > 0 and g_s.abs().max() > 0
    # no_grad and the (S, N, 3) form give the forward's bytes
    assert _eq(decode_color_batch(dec_c, cc, sc, pts, counts=SIZES, no_grad=True), y)
    cube = pts[:6 * 50].reshape(6, 50, 3)
    assert _eq(decode_color_batch(dec_c, cc, sc, cube).reshape(-1, 3), decode_color_batch(dec_c, cc, sc, cube.reshape(-1, 3), counts=[50] * 6))


def test_segmented_decode_two_chunks(color_case):
    """S = 65: the 65th segment runs in a second launch sequence, with its own code rows and point offset."""
    import torch
    from core.utils.decoder_utils import decode_color_batch
    dec_c, cc, sc, pts, w = color_case
    sizes = [(7 * i) % 9 for i in range(64)] + [70]                 # 0..8 points each, then more than one tile in the second chunk
    n = sum(sizes)
    assert n <= pts.shape[0]
    rs = np.random.RandomState(5)
    ccs = cc[torch.from_numpy(rs.randint(0, 6, 65)).cuda()] + torch.arange(65, device='cuda', dtype=torch.float32)[:, None] * 1e-3
    scs = sc[torch.from_numpy(rs.randint(0, 6, 65)).cuda()]
    c, s, x = ccs.clone().requires_grad_(True), scs.clone().requires_grad_(True), pts[:n].clone().requires_grad_(True)
    y = decode_color_batch(dec_c, c, s, x, counts=sizes)
    (y * w[:n]).sum().backward()
    for k, a, b in _segments(sizes):
        if a == b:
            assert not c.grad[k].any() and not s.grad[k].any()
            continue
        if k % 8 and k < 63:                                        # every eighth segment and the two around the chunk border
            continue
        y1, c1, s1, x1 = _single(dec_c, ccs[k:k + 1], scs[k:k + 1], pts[a:b], w[a:b])
        assert _eq(y[a:b], y1) and _eq(x.grad[a:b], x1) and _eq(c.grad[k:k + 1], c1) and _eq(s.grad[k:k + 1], s1), k


def test_segmented_decode_shared_codes(color_case):
    """latent_stride 0: one [shape | colour] pair for every segment; the code gradient still has one row per segment, each the
    stand-alone call's, and the autograd node hands the shared codes the sum of the rows."""
    import torch
    from core.utils.decoder_utils import decode_color_batch
    from distr import functions
    dec_c, cc, sc, pts, w = color_case
    eng = functions.get_color_engine(dec_c, 0)
    c0, s0 = cc[2:3], sc[4:5]
    out = functions.color_eval_multi(eng, c0, s0, pts, SIZES)
    g_rows, g_x = functions.color_backward_multi(eng, c0, s0, pts, SIZES, w)
    assert g_rows.shape == (len(SIZES), 256 + CS)
    for s, a, b in _segments(SIZES):
        if a == b:
            assert not g_rows[s].any()
            continue
        y1, c1, s1, x1 = _single(dec_c, c0, s0, pts[a:b], w[a:b])
        assert _eq(out[a:b], y1) and _eq(g_x[a:b], x1) and _eq(g_rows[s:s + 1, 256:], c1) and _eq(g_rows[s:s + 1, :256], s1), s
    c, s = c0.clone().requires_grad_(True), s0.clone().requires_grad_(True)
    (decode_color_batch(dec_c, c, s, pts, counts=SIZES) * w).sum().backward()
    assert _eq(c.grad, g_rows[:, 256:].sum(0, keepdim=True)) and _eq(s.grad, g_rows[:, :256].sum(0, keepdim=True))


# ------------------------------------------------------------------------------------------ the batch of views
def _cameras():
    from distr import fixture
    Rs, Ts = zip(*[fixture.make_camera(*c) for c in CAMS])
    Rs, Ts = list(Rs), list(Ts)
    Rs.append(Rs[0].copy())                                          # the fourth view looks past the shape: the unit sphere is outside its image
    Ts.append(np.array([4.0, 0.0, 1.6], dtype=np.float32))
    return np.stack(Rs).astype(np.float32), np.stack(Ts).astype(np.float32)


@pytest.fixture(scope='module')
def scene(fixture_decoder):
    """The renderer (F1, 48 x 45, 30 steps), the four cameras, a code pair per view, weights on every output -- and every view's own
    B = 1 render_batch with its gradients, plain and lit, computed once and shared by the tests below."""
    import torch
    from core.sdfrenderer import SDFRenderer_color
    from distr import fixture
    dec, dec_c, latent, code = _decoders(fixture_decoder, CS)
    r = SDFRenderer_color(dec, dec_c, fixture.make_intrinsic(H, W), img_hw=(H, W), march_step=30, buffer_size=2)
    Rs, Ts = _cameras()
    B = Rs.shape[0]
    rs = np.random.RandomState(11)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()
    sc = t(latent + 0.15 * np.abs(latent).max() * rs.standard_normal((B, 256)))
    cc = t(code + 0.3 * np.abs(code).max() * rs.standard_normal((B, CS)))
    sc[0], cc[0] = t(latent)[0], t(code)[0]
    wts = dict(d=t(rs.rand(B, H, W)), n=t(rs.standard_normal((B, H, W, 3))), c=t(rs.standard_normal((B, H, W, 3))), q=t(rs.rand(B, H, W)))
    S = dict(r=r, Rs=t(Rs), Ts=t(Ts), B=B, sc=sc, cc=cc, w=wts, lights=t(LIGHTS), energies=t(ENERGIES))
    S['single'] = {}
    for lit in (False, True):
        for shared in (False, True):
            for v in range(B):
                S['single'][(lit, shared, v)] = _run_batch(S, [v], lit, shared)
    return S


def _light_kw(S, lit, views=None):
    if not lit:
        return {}
    return dict(lighting_locations=S['lights'], lighting_energies=S['energies'])


def _loss(S, outs, views):
    d, n, col, m, q = outs
    w = S['w']
    v = torch_index(views)
    return (d * w['d'][v])[m.bool()].sum() + (n * w['n'][v]).sum() + (col * w['c'][v]).sum() + (q * w['q'][v]).sum()


def torch_index(views):
    import torch
    return torch.tensor(list(views), device='cuda')


def _run_batch(S, views, lit, shared, only=None):
    """render_batch of `views` + one backward of the weighted loss (only: the loss of that batch row alone). Shared codes are view 0's
    pair. Returns the five outputs and the four gradients (codes: one row per view unless shared)."""
    v = torch_index(views)
    cc = (S['cc'][:1] if shared else S['cc'][v]).clone().requires_grad_(True)
    sc = (S['sc'][:1] if shared else S['sc'][v]).clone().requires_grad_(True)
    Rs, Ts = S['Rs'][v].clone().requires_grad_(True), S['Ts'][v].clone().requires_grad_(True)
    outs = S['r'].render_batch(cc, sc, Rs, Ts, **_light_kw(S, lit))
    if only is None:
        _loss(S, outs, views).backward()
    else:
        _loss(S, tuple(o[only:only + 1] for o in outs), views[only:only + 1]).backward()
    return dict(out=tuple(o.detach() for o in outs), g_cc=cc.grad, g_sc=sc.grad, g_R=Rs.grad, g_T=Ts.grad)


def test_view_counts_cover_the_edges(scene):
    counts = [int(scene['single'][(False, False, v)]['out'][3].sum()) for v in range(scene['B'])]
    print('valid pixels per view:', counts)
    assert counts[3] == 0 and all(c > 0 and c % 64 != 0 for c in counts[:3]), counts
    assert len(set(counts)) == 4


def test_stage_points_and_colours_are_the_single_paths(scene):
    """The index and point list the forward hands back: the index is nonzero(mask) in row-major order, and color_eval on each view's
    points gives that view's colours byte for byte."""
    import torch
    from distr import functions
    S = scene
    r, B = S['r'], S['B']
    with torch.no_grad():
        cfg = r._cfg(0.1, 'recursive', True, want_normal=True)
        cfg.use_depth2normal = 0
        z, mask, _, _, _ = functions.render_batch_call(r._engine, cfg, S['sc'], S['Rs'], S['Ts'])
        ceng = r._color_engine
        rgb, sv = functions.color_stage_forward(ceng, cfg, S['cc'], S['sc'], S['Rs'], S['Ts'], z, mask, want_lists=True)
        assert rgb.shape == (B, H, W, 3)
        for v in range(B):
            idx = torch.nonzero(mask[v]).reshape(-1)
            n = int(sv['totals'][v])
            assert n == idx.numel()
            assert torch.equal(sv['index'][v, :n].long(), idx)
            want = torch.zeros(H * W, 3, device='cuda')
            if n:
                col = functions.color_eval(ceng, S['cc'][v:v + 1], S['sc'][v:v + 1], sv['xyz'][v, :n])
                want = want.index_copy(0, idx, col)
            assert _eq(rgb[v].reshape(-1, 3), want), v
            assert _eq(rgb[v], S['single'][(False, False, v)]['out'][2][0])
        assert int(sv['totals'][3]) == 0 and int(sv['totals'].max()) > 64


@pytest.mark.parametrize('lit', [False, True], ids=['plain', 'lit'])
@pytest.mark.parametrize('shared', [True, False], ids=['shared_codes', 'code_per_view'])
def test_batch_equals_standalone(scene, shared, lit):
    """B = 4: every view's five outputs and gradients are byte-identical to its own B = 1 call; depth, normal, mask and min_sdf also to
    `render` of that view; a second run gives the same bytes."""
    import torch
    S = scene
    B = S['B']
    views = list(range(B))
    a, b = _run_batch(S, views, lit, shared), _run_batch(S, views, lit, shared)
    for k in ('g_cc', 'g_sc', 'g_R', 'g_T'):
        assert _eq(a[k], b[k]), k
    assert all(_eq(x, y) for x, y in zip(a['out'], b['out']))
    for v in views:
        one = S['single'][(lit, shared, v)]
        for i, name in enumerate(('depth', 'normal', 'color', 'mask', 'min_sdf')):
            assert _eq(a['out'][i][v:v + 1], one['out'][i]), (v, name)
        # a shared pair's gradient is the sum over the views: view v's own term is the backward of view v's loss alone
        g = _run_batch(S, views, lit, shared, only=v) if shared else a
        row = slice(0, 1) if shared else slice(v, v + 1)
        assert _eq(g['g_cc'][row], one['g_cc']) and _eq(g['g_sc'][row], one['g_sc']), v
        assert _eq(g['g_R'][v:v + 1], one['g_R']) and _eq(g['g_T'][v:v + 1], one['g_T']), v
        with torch.no_grad():
            cc, sc = (S['cc'][:1], S['sc'][:1]) if shared else (S['cc'][v:v + 1], S['sc'][v:v + 1])
            d, n, col, m, q = S['r'].render(cc, sc, S['Rs'][v], S['Ts'][v])      # (its geometry does not depend on the lights)
        assert _eq(a['out'][0][v], d) and _eq(a['out'][1][v], n) and _eq(a['out'][3][v], m) and _eq(a['out'][4][v], q), v
    empty = S['single'][(lit, shared, 3)]
    assert not a['out'][2][3].any() and not a['out'][3][3].any()
    assert not empty['g_cc'].any() and float(one['g_cc'].abs().max()) == 0.0
    assert float(S['single'][(lit, shared, 0)]['g_cc'].abs().max()) > 0 and float(S['single'][(lit, shared, 1)]['g_T'].abs().max()) > 0


@pytest.mark.parametrize('terms', ['all_outputs', 'colour_only'])
@pytest.mark.parametrize('M', [1, 3])
def test_against_the_composed_path(scene, M, terms):
    """The same views, lit with M lights, against `render` + backward view by view. Colours: p99 <= 1e-4 on the common mask (the points
    are formed in another f32 order). Gradients: <= 1e-4 of each gradient's largest entry, the bar for reduction-order differences --
    for the loss over every output and for the colour term alone (in the full loss the geometry's camera gradient is the larger part;
    alone, every entry is the colour stage's: decoder, points, shading, and the normal image's gradient through the render node)."""
    import torch
    S = scene
    r, B = S['r'], S['B']
    kw = dict(lighting_locations=S['lights'][:M], lighting_energies=S['energies'][:M])
    views = list(range(B))
    cc, sc = S['cc'].clone().requires_grad_(True), S['sc'].clone().requires_grad_(True)
    Rs, Ts = S['Rs'].clone().requires_grad_(True), S['Ts'].clone().requires_grad_(True)
    outs = r.render_batch(cc, sc, Rs, Ts, **kw)
    loss = _loss if terms == 'all_outputs' else (lambda S_, o, vs: (o[2] * S_['w']['c'][torch_index(vs)]).sum())
    loss(S, outs, views).backward()
    worst = {}
    for v in range(3):
        c1, s1 = S['cc'][v:v + 1].clone().requires_grad_(True), S['sc'][v:v + 1].clone().requires_grad_(True)
        R1, T1 = S['Rs'][v].clone().requires_grad_(True), S['Ts'][v].clone().requires_grad_(True)
        d, n, col, m, q = r.render(c1, s1, R1, T1, **kw)
        loss(S, tuple(o[None] for o in (d, n, col, m, q)), [v]).backward()
        both = (m.bool() & outs[3][v].bool()).cpu().numpy()
        assert torch.equal(m, outs[3][v])
        dc = np.abs(col.detach().cpu().numpy() - outs[2][v].detach().cpu().numpy())[both]
        worst[('color_p99', v)] = float(np.percentile(dc, 99))
        for k, got, want in (('g_color_code', cc.grad[v], c1.grad[0]), ('g_latent', sc.grad[v], s1.grad[0]), ('g_R', Rs.grad[v], R1.grad),
                             ('g_T', Ts.grad[v], T1.grad)):
            worst[(k, v)] = float((got - want).abs().max() / want.abs().max())
    print('render_batch against render, M = %d, %s:' % (M, terms), {('%s[%d]' % k): '%.2e' % x for k, x in sorted(worst.items())})
    for k, x in worst.items():
        assert x <= 1e-4, (k, x)


def test_relight_frames_equal_lit_renders(scene):
    """F = 3 frames of one view equal three lit render_batch colour images of that view, byte for byte."""
    import torch
    S = scene
    r = S['r']
    frames = torch.stack([S['lights'], S['lights'].flip(0) * 1.3, S['lights'][[1, 2, 0]] - 0.4])          # (3, M = 3, 3)
    en = torch.stack([S['energies'], S['energies'].flip(0), S['energies'] * 0.5])
    v = 1
    with torch.no_grad():
        cc, sc, Rv, Tv = S['cc'][v:v + 1], S['sc'][v:v + 1], S['Rs'][v], S['Ts'][v]
        d, n, col, m, q = r.render_batch(cc, sc, Rv[None], Tv[None])
        z, _, _ = r.render_depth(sc, Rv, Tv)
        out = r.relight(col[0], n[0], z, m[0], Rv, Tv, frames, en)
        assert out.shape == (3, H, W, 3)
        for f in range(3):
            lit = r.render_batch(cc, sc, Rv[None], Tv[None], lighting_locations=frames[f], lighting_energies=en[f])[2][0]
            assert _eq(out[f], lit), f
            assert float((out[f] - col[0]).abs().max()) > 1e-3
        assert _eq(r.relight(col[0], n[0], z, m[0], Rv, Tv, frames)[1],
                   r.render_batch(cc, sc, Rv[None], Tv[None], lighting_locations=frames[1])[2][0])       # default energies: ones
    assert not out.requires_grad


# ------------------------------------------------------------------------------------------ 3. goldens through render_batch, B = 1
def _golden_renderer(fixture_decoder, g):
    from core.sdfrenderer import SDFRenderer_color
    dec, dec_c, _, code = _decoders(fixture_decoder, int(g['color_size']))
    Hg, Wg = int(g['H']), int(g['W'])
    return SDFRenderer_color(dec, dec_c, g['K'], img_hw=(Hg, Wg), march_step=int(g['march_step']), buffer_size=int(g['buffer_size']))


def test_g10_through_render_batch(fixture_decoder):
    """G10's scene, plain and lit, with the bars of test_color_render_matches_reference_golden."""
    import torch
    g = dict(np.load(os.path.join(GOLDEN, 'g10_color_render.npz')))
    r = _golden_renderer(fixture_decoder, g)
    c = lambda k: torch.from_numpy(g[k]).cuda()
    d, n, col, m, q = (o[0] for o in r.render_batch(c('color_code'), c('latent'), c('R')[None], c('T')[None], no_grad=True))
    mm = m.cpu().numpy().astype(bool)
    both = mm & g['mask'].astype(bool)
    assert (mm != g['mask'].astype(bool)).sum() <= 1
    assert np.abs(d.cpu().numpy() - g['depth'])[both].max() <= 1e-4
    assert np.abs(q.cpu().numpy() - g['min_sdf']).max() <= 1e-4
    assert np.percentile(np.abs(n.cpu().numpy() - g['normal'])[both], 99) <= 1e-4
    assert np.percentile(np.abs(col.cpu().numpy() - g['color'])[both], 99) <= 1e-4
    col2 = r.render_batch(c('color_code'), c('latent'), c('R')[None], c('T')[None], no_grad=True, lighting_locations=c('lights'),
                          lighting_energies=c('energies'))[2][0]
    assert np.percentile(np.abs(col2.cpu().numpy() - g['color_shaded'])[both], 99) <= 1e-4


def test_g26_through_render_batch(fixture_decoder):
    """G26's scene with the bars of test_color_render_gradients_match_reference_golden: loss and gradients w.r.t. colour code, shape
    code, R and T, plain and lit; then its no_grad block as it stands."""
    import torch
    g = dict(np.load(os.path.join(GOLDEN, 'g26_color_render_grad.npz')))
    r = _golden_renderer(fixture_decoder, g)
    c = lambda k: torch.from_numpy(g[k]).cuda()
    for tag in ('plain', 'lit'):
        lat, cc = c('latent').requires_grad_(True), c('color_code').requires_grad_(True)
        Rt, Tt = c('R').requires_grad_(True), c('T').requires_grad_(True)
        kw = {} if tag == 'plain' else dict(lighting_locations=c('lights'), lighting_energies=c('energies'))
        d, n, col, m, q = (o[0] for o in r.render_batch(cc, lat, Rt[None], Tt[None], **kw))
        mb = m.bool()
        assert int((m.cpu().numpy() != g[tag + '.mask']).sum()) <= 1
        both = mb.cpu().numpy() & g[tag + '.mask'].astype(bool)
        assert np.abs(d.detach().cpu().numpy() - g[tag + '.depth'])[both].max() <= 1e-4
        assert np.abs(q.detach().cpu().numpy() - g[tag + '.q']).max() <= 1e-4
        assert np.percentile(np.abs(n.detach().cpu().numpy() - g[tag + '.normal'])[both], 99) <= 1e-4
        assert np.percentile(np.abs(col.detach().cpu().numpy() - g[tag + '.color'])[both], 99) <= 1e-4
        L = (d * c('w_d'))[mb].sum() + (n * c('w_n')).sum() + (col * c('w_c')).sum() + (q * c('w_q')).sum()
        L.backward()
        assert abs(float(L.detach()) - float(g[tag + '.loss'])) <= 5e-5 * abs(float(g[tag + '.loss']))
        res = {}
        for k, t in (('g_color_code', cc), ('g_latent', lat), ('g_R', Rt), ('g_T', Tt)):
            ref = g['%s.%s' % (tag, k)]
            res[k] = float(np.abs(t.grad.cpu().numpy().reshape(-1) - ref.reshape(-1)).max() / np.abs(ref).max())
            assert res[k] <= max(1e-3, 2.0 * float(g['%s.%s_floor_rel' % (tag, k)])), (tag, k, res[k])
        print('G26 through render_batch', tag, {k: '%.1e' % v for k, v in res.items()})
    lat, cc, Rt = c('latent').requires_grad_(True), c('color_code').requires_grad_(True), c('R').requires_grad_(True)
    d, n, col, m, q = r.render_batch(cc, lat, Rt[None], c('T')[None], no_grad=True)
    assert not col.requires_grad and not d.requires_grad and not q.requires_grad and n.requires_grad
    n.sum().backward()
    assert (lat.grad is None or float(lat.grad.abs().max()) == 0.0) and cc.grad is None and float(Rt.grad.abs().max()) > 0


# ------------------------------------------------------------------------------------------ 7. refusals
def test_refusals(scene, engine):
    import torch
    from distr import binding, functions
    S = scene
    r = S['r']
    cc, sc, Rs, Ts = S['cc'], S['sc'], S['Rs'], S['Ts']
    # a context without a colour decoder
    with pytest.raises(binding.DistrError, match='distr_set_color_decoder has not been called'):
        functions.color_eval_multi(_NoColor(engine), cc[:1], sc[:1], torch.zeros(3, 3, device='cuda'), [3])
    cfg = r._cfg(0.1, 'recursive', True, want_normal=True)
    with pytest.raises(binding.DistrError, match='distr_set_color_decoder has not been called'):
        functions.color_stage_forward(_NoColor(engine), cfg, cc, sc, Rs, Ts, torch.zeros(4, H * W, device='cuda'), torch.zeros(4, H * W, dtype=torch.uint8, device='cuda'))
    # codes of the wrong length or row count
    with pytest.raises(ValueError, match=r'shape codes \(1, 256\) or \(4, 256\) and colour codes \(1, 32\) or \(4, 32\)'):
        r.render_batch(cc[:, :31], sc, Rs, Ts)
    with pytest.raises(ValueError, match=r'shape codes \(1, 256\) or \(4, 256\)'):
        r.render_batch(cc, sc[:3], Rs, Ts)
    with pytest.raises(ValueError, match=r'shape codes \(1, 256\) or \(4, 256\)'):
        r.render_batch(cc, sc[:, :200], Rs, Ts)
    # lights are observations
    with pytest.raises(ValueError, match='lighting_locations requires grad'):
        r.render_batch(cc, sc, Rs, Ts, lighting_locations=S['lights'].clone().requires_grad_(True))
    with pytest.raises(ValueError, match='lighting_energies requires grad'):
        r.render_batch(cc, sc, Rs, Ts, lighting_locations=S['lights'], lighting_energies=S['energies'].clone().requires_grad_(True))
    with pytest.raises(ValueError, match=r'expected \(M, 3\) or \(4, M, 3\)'):
        r.render_batch(cc, sc, Rs, Ts, lighting_locations=S['lights'][None].expand(3, -1, -1))
    # cameras
    with pytest.raises(ValueError, match='of the same B'):
        r.render_batch(cc, sc, Rs, Ts[:3])
    with pytest.raises(ValueError, match='of the same B'):
        r.render_batch(cc[:1], sc[:1], [Rs[0], Rs[1]], [Ts[0]])
    with pytest.raises(ValueError, match=r'relight takes \(F, M, 3\)'):
        r.relight(torch.zeros(H, W, 3, device='cuda'), torch.zeros(H, W, 3, device='cuda'), torch.zeros(H * W, device='cuda'),
                  torch.zeros(H, W, device='cuda'), Rs[0], Ts[0], S['lights'])


class _NoColor(object):
    """An engine whose context holds the SDF decoder only, with the colour decoder's code length: what reaches the library is a call on a
    context that distr_set_color_decoder never saw."""

    def __init__(self, engine):
        self.ctx, self.device, self.latent_size = engine.ctx, engine.device, 256 + CS
