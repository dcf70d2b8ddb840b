"""Weight gradients of the colour decoder through the colour render on the GPU: the export of the colour stage's
decoder list (distr_color_stage_samples_export_batch), the layer-wise train path run over it (functions.color_stage_weight_grads, the
optional trailing weights of ColorStageFunction) and SDFRenderer_color(color_decoder_grad=True).

Expected values never come from the code under test, except where a test says so (the consistency checks of the batch form): the list is
the forward's own `want_lists` output and numpy's gather of the upstream, the shading term is distr_color_relight of an all-ones colour
image, the weight gradients are tests/color_train_restatement.gradients in float64 over the exported list on the ReLU gates the train path
saved. The stage runs on synthetic zdepth / mask buffers of 48 x 48 pixels (two compaction blocks of MTILE = 2048 per view) so that the
valid counts sit on every edge; every stage run and float64 gradient is made once per module and not modified."""
import ctypes as C
import copy

import numpy as np
import pytest

import color_train_restatement as ctr

pytestmark = pytest.mark.gpu

GUARD = 4096
BAR = 1e-4              # the project's bar for another f32 summation order, of a block's largest entry (sections 8f-8i)
H = W = 48
P = H * W
CS = 32
EDGE_COUNTS = [0, 1, 63, 64, 65, 2048, 2049]
LIGHTS = np.array([[1.5, 2.0, -1.0], [-2.0, 0.5, 2.5], [0.3, -2.5, -2.0]], dtype=np.float32)
ENERGIES = np.array([0.9, 0.6, 0.4], dtype=np.float32)


def _t(a, dtype=np.float32):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _guarded(nbytes):
    import torch
    buf = torch.empty(nbytes + 2 * GUARD, dtype=torch.uint8, device='cuda')
    buf[:GUARD] = 0xA5
    buf[GUARD:GUARD + nbytes] = 0xFF
    buf[GUARD + nbytes:] = 0xA5
    return buf


def _whole(buf, nbytes):
    return bool((buf[:GUARD] == 0xA5).all()) and bool((buf[GUARD + nbytes:] == 0xA5).all())


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ------------------------------------------------------------------------------------------------ the colour decoder and the synthetic views
@pytest.fixture(scope='module')
def color(fixture_decoder):
    """(colour module f32 on the GPU, its engine, Wc, bc, colour code (1, cs), shape code (1, 256), cfg of 48 x 48)"""
    import torch
    from distr import binding, fixture, functions
    Wc, bc, code = fixture.make_color_decoder_weights(color_size=CS)
    dec = ctr.color_module(Wc, bc, dtype=torch.float32).cuda()
    cfg = binding.make_cfg((H, W), fixture.make_intrinsic(H, W), marcher='recursive')
    return dict(dec=dec, eng=functions.get_color_engine(dec, 0), Wc=Wc, bc=bc, code=np.asarray(code, np.float32).reshape(1, CS),
                latent=np.asarray(fixture_decoder[2], np.float32).reshape(1, 256), cfg=cfg)


def make_views(counts, seed):
    """Synthetic inputs of the stage for len(counts) views: masks with exactly counts[v] valid pixels (the first and the last pixel among
    them where the count allows), ray-length depths in [1, 2), unit normals, cameras around the origin, an upstream gradient."""
    from distr import fixture
    rs = np.random.RandomState(seed)
    B = len(counts)
    mask = np.zeros((B, P), np.uint8)
    for v, c in enumerate(counts):
        idx = rs.choice(np.arange(1, P - 1), max(c - 2, 0), replace=False)
        mask[v, idx] = 1
        if c >= 1:
            mask[v, P - 1] = 1
        if c >= 2:
            mask[v, 0] = 1
        assert int(mask[v].sum()) == c
    z = (1.0 + rs.rand(B, P)).astype(np.float32)
    n = rs.standard_normal((B, H, W, 3))
    n = (n / np.linalg.norm(n, axis=-1, keepdims=True)).astype(np.float32)
    cams = [fixture.make_camera(25.0 * v - 60.0, 10.0 + 3.0 * v, 1.5 + 0.05 * v, 4.0 * v) for v in range(B)]
    return dict(B=B, counts=list(counts), mask=mask, z=z, normal=n, R=np.stack([c[0] for c in cams]).astype(np.float32),
                T=np.stack([c[1] for c in cams]).astype(np.float32), g_rgb=rs.standard_normal((B, H, W, 3)).astype(np.float32))


def codes_for(color, B, own, seed=3):
    rs = np.random.RandomState(seed)
    if not own:
        return color['code'], color['latent']
    return ((color['code'] + 0.3 * np.abs(color['code']).max() * rs.standard_normal((B, CS))).astype(np.float32),
            (color['latent'] + 0.15 * np.abs(color['latent']).max() * rs.standard_normal((B, 256))).astype(np.float32))


class Stage(object):
    """One distr_color_stage_forward_batch on the views `vs` (a subset by `rows`), its backward on g_rgb with every output asked for, and
    the export into arrays that lie between 0xA5 guards and are pre-filled with 0xFF."""

    def __init__(self, color, vs, cc, sc, lit, rows=None):
        from distr import functions
        rows = list(range(vs['B'])) if rows is None else list(rows)
        self.color, self.B, self.lit = color, len(rows), lit
        pick = lambda a: a if a.shape[0] == 1 else a[rows]
        self.vs = {k: (v[rows] if isinstance(v, np.ndarray) else v) for k, v in vs.items()}
        kw = dict(normal=_t(self.vs['normal']), lights=_t(LIGHTS), energies=_t(ENERGIES)) if lit else {}
        self.rgb, self.sv = functions.color_stage_forward(color['eng'], color['cfg'], _t(pick(cc)), _t(pick(sc)), _t(self.vs['R']), _t(self.vs['T']),
                                                          _t(self.vs['z']), _t(self.vs['mask'], np.uint8), want_lists=True, **kw)
        self.ws_b = None

    def backward(self, decoder=True):
        """-> dict of numpy g_lat (B, 256 + cs), g_R, g_T, g_n (lit); the backward workspace stays in self.ws_b"""
        import torch
        from distr import binding
        eng, cfg, sv, B = self.color['eng'], self.color['cfg'], self.sv, self.B
        Rc, Tc, z, n = sv['views']
        loc, en, st = sv['lights']
        nan = lambda *s: torch.full(s, float('nan'), dtype=torch.float32, device='cuda')
        g = _t(self.vs['g_rgb']).reshape(-1)
        g_lat, g_R, g_T = (nan(B, eng.latent_size) if decoder else None), nan(B, 9), nan(B, 3)
        g_n = nan(B, H, W, 3) if self.lit else None
        self.ws_b = torch.full((sv['bwd_bytes'],), 0xFF, dtype=torch.uint8, device='cuda')
        p = binding.ptr
        eng.ctx.check(eng.ctx.L.distr_color_stage_backward_batch(
            eng.ctx.h, C.byref(cfg), B, p(Rc), p(Tc), p(z), p(n), p(sv['lat']), sv['stride'], None if st is None else C.byref(st), p(sv['ws']),
            sv['ws'].numel(), p(g), p(g_lat), p(g_R), p(g_T), p(g_n), p(self.ws_b), self.ws_b.numel(), eng.ctx.stream()))
        torch.cuda.synchronize()
        return {k: (None if t is None else t.cpu().numpy()) for k, t in (('g_lat', g_lat), ('g_R', g_R), ('g_T', g_T), ('g_n', g_n))}

    def export(self, extra=0):
        """-> (per view (xyz (n, 3), up (n, 3), index (n,)), counts). cap = P + extra. Asserts whole guards, untouched bytes behind every
        count, that a call without index writes the same xyz / up bytes, and that functions.color_stage_samples agrees."""
        import torch
        from distr import functions
        eng, cfg, sv, B = self.color['eng'], self.color['cfg'], self.sv, self.B
        cap = P + extra
        sizes = dict(xyz=B * cap * 12, up=B * cap * 12, index=B * cap * 4, counts=B * 4)
        raws = []
        for with_index in (True, False):
            bufs = {k: _guarded(n) for k, n in sizes.items()}
            at = lambda k: C.c_void_p(bufs[k].data_ptr() + GUARD)
            eng.ctx.check(eng.ctx.L.distr_color_stage_samples_export_batch(
                eng.ctx.h, C.byref(cfg), B, C.c_void_p(sv['ws'].data_ptr()), sv['ws'].numel(), C.c_void_p(self.ws_b.data_ptr()), self.ws_b.numel(),
                at('xyz'), at('up'), at('index') if with_index else None, cap, at('counts'), eng.ctx.stream()))
            torch.cuda.synchronize()
            for k, n in sizes.items():
                assert _whole(bufs[k], n), 'a guard of the %s array was written' % k
            raws.append({k: bufs[k][GUARD:GUARD + n].cpu().numpy() for k, n in sizes.items()})
        raw, raw2 = raws
        assert raw['xyz'].tobytes() == raw2['xyz'].tobytes() and raw['up'].tobytes() == raw2['up'].tobytes() and (raw2['index'] == 0xFF).all()
        counts = raw['counts'].view(np.int32)
        assert (counts >= 0).all() and (counts <= P).all(), counts
        xyz, up, index = raw['xyz'].reshape(B, cap * 12), raw['up'].reshape(B, cap * 12), raw['index'].reshape(B, cap * 4)
        views = []
        for v in range(B):
            n = int(counts[v])
            assert (xyz[v, n * 12:] == 0xFF).all() and (up[v, n * 12:] == 0xFF).all() and (index[v, n * 4:] == 0xFF).all(), 'rows at or beyond the count were written'
            views.append((xyz[v, :n * 12].view(np.float32).reshape(n, 3).copy(), up[v, :n * 12].view(np.float32).reshape(n, 3).copy(),
                          index[v, :n * 4].view(np.int32).copy()))
        x2, u2, i2, n2 = functions.color_stage_samples(eng, cfg, sv, self.ws_b)
        assert np.array_equal(n2.cpu().numpy(), counts)
        for v in range(B):
            n = int(counts[v])
            assert np.array_equal(_bits(x2[v, :n].cpu().numpy()), _bits(views[v][0])) and np.array_equal(_bits(u2[v, :n].cpu().numpy()), _bits(views[v][1]))
            assert np.array_equal(i2[v, :n].cpu().numpy(), views[v][2])
        return views, counts


def shading(color, vs, v):
    """The shading term s of every pixel of view v (zero off the mask): distr_color_relight of an all-ones colour image, 1.0f * s = s."""
    import torch
    from distr import functions
    out = functions.color_relight(color['eng'], color['cfg'], torch.ones(H, W, 3, device='cuda'), _t(vs['normal'][v]), _t(vs['z'][v]),
                                  _t(vs['mask'][v], np.uint8), _t(vs['R'][v]), _t(vs['T'][v]), _t(LIGHTS)[None], _t(ENERGIES))
    s = out[0].cpu().numpy()
    assert np.array_equal(_bits(s[..., 0]), _bits(s[..., 1])) and np.array_equal(_bits(s[..., 0]), _bits(s[..., 2]))
    return s[..., 0].reshape(P)


# ------------------------------------------------------------------------------------------------ 1: the export at every edge
@pytest.fixture(scope='module')
def edge_views():
    return make_views(EDGE_COUNTS, 35)


@pytest.mark.parametrize('lit', [False, True], ids=['unlit', 'lit'])
def test_export_at_the_count_edges(color, edge_views, lit):
    """Counts 0, 1, 63, 64, 65, MTILE, MTILE + 1: xyz equals the forward's own list bit for bit, counts the totals, the index the valid
    pixels in row-major order; up = g_rgb[index] (unlit) or g_rgb[index] * s as ONE f32 product (lit), bit for bit; all of it between
    whole guards, nothing at or beyond a count written, with the row stride cap = P and cap = P + 3."""
    vs = edge_views
    cc, sc = codes_for(color, vs['B'], own=True)
    st = Stage(color, vs, cc, sc, lit)
    st.backward()
    for extra in (0, 3):
        views, counts = st.export(extra)
        assert list(counts) == EDGE_COUNTS and np.array_equal(st.sv['totals'].cpu().numpy(), counts)
        for v, (xyz, up, index) in enumerate(views):
            n = int(counts[v])
            assert np.array_equal(index, np.nonzero(vs['mask'][v])[0].astype(np.int32)), v
            assert np.array_equal(index, st.sv['index'][v, :n].cpu().numpy()), v
            assert np.array_equal(_bits(xyz), _bits(st.sv['xyz'][v, :n].cpu().numpy())), v
            g = vs['g_rgb'][v].reshape(P, 3)[index]
            want = g * shading(color, vs, v)[index][:, None] if lit else g          # (f32 * f32 in numpy: one rounding, as the kernel's)
            assert want.dtype == np.float32 and np.array_equal(_bits(up), _bits(want)), (v, 'up', int((_bits(up) != _bits(want)).sum()))
            if lit and n:
                assert np.abs(want - g).max() > 0, 'the shading term should move the upstream'


# ------------------------------------------------------------------------------------------------ 2: the views of a batch
@pytest.mark.parametrize('lit', [False, True], ids=['unlit', 'lit'])
@pytest.mark.parametrize('own', [False, True], ids=['shared_codes', 'own_codes'])
def test_batch_views_equal_their_own_call(color, own, lit):
    """B = 4 with one empty view: every view's exported rows and its code, camera and normal gradients are, byte for byte, those of its
    own B = 1 call (expected values from the code under test: a consistency check of the batch form)."""
    vs = make_views([700, 0, 65, 2100], 36)
    cc, sc = codes_for(color, 4, own)
    batch = Stage(color, vs, cc, sc, lit)
    gb = batch.backward()
    got, counts = batch.export()
    assert list(counts) == vs['counts']
    for v in range(4):
        alone = Stage(color, vs, cc, sc, lit, rows=[v])
        ga = alone.backward()
        exp, c1 = alone.export()
        assert int(c1[0]) == vs['counts'][v]
        assert alone.rgb.cpu().numpy().tobytes() == batch.rgb[v:v + 1].cpu().numpy().tobytes()
        for name, a, b in zip(('xyz', 'up', 'index'), got[v], exp[0]):
            assert a.shape == b.shape and a.tobytes() == b.tobytes(), (v, name)
        for k in ('g_lat', 'g_R', 'g_T') + (('g_n',) if lit else ()):
            assert gb[k][v:v + 1].tobytes() == ga[k].tobytes(), (v, k)
    assert not gb['g_lat'][1].any() and np.isfinite(gb['g_lat']).all() and np.abs(gb['g_lat'][0]).max() > 0


# ------------------------------------------------------------------------------------------------ 3: the weight gradients against float64
def _weights(color):
    return [_t(a) for a in list(color['Wc']) + list(color['bc'])]


def _gpu_gates(weights, lat, pts_per_view):
    """The ReLU pattern the train path saves on the views' lists (one segment per view with points), eight boolean tensors in list order."""
    import torch
    from distr import functions
    views = [v for v, x in enumerate(pts_per_view) if len(x)]
    cnt = [len(pts_per_view[v]) for v in views]
    codes = lat if lat.shape[0] == 1 else lat[views]
    _, saved = functions.train_forward(weights, codes, _t(np.concatenate([pts_per_view[v] for v in views])), cnt, net=functions.color_train_net(weights))
    idx = torch.cat([torch.arange(*saved.rows(s)) for s in range(len(cnt))]).cuda()
    return [(saved.activations(l + 1)[idx] > 0).cpu() for l in range(8)], views, cnt


def _assert_blocks(tag, got, ref_W, ref_b):
    blocks = ctr.blockwise_residuals([g.cpu().numpy() for g in got], [t.numpy() for t in list(ref_W) + list(ref_b)], CS)
    worst = max(blocks, key=lambda t: t[1])
    print('%s: worst block %s %.3e (largest entry %.3e)' % (tag, worst[0], worst[1], worst[2]))
    assert all(top > 0 for _, _, top in blocks), [b for b in blocks if not b[2] > 0]
    assert worst[1] <= BAR, (tag, worst)
    return worst[1]


@pytest.mark.parametrize('own', [False, True], ids=['shared_codes', 'own_codes'])
@pytest.mark.parametrize('lit', [False, True], ids=['unlit', 'lit'])
def test_weight_gradients_match_float64_on_the_exported_list(color, lit, own):
    """color_stage_weight_grads on the workspaces of a backward of three views (one empty) against float64 gradients over the exported
    list (pinned above), every ReLU on the gate the train path saved: 1e-4 of each block's largest entry. The layer-wise code gradient of
    every view agrees with float64 and with the fused backward's to the same bar."""
    import torch
    from distr import functions
    vs = make_views([65, 0, 700], 37)
    cc, sc = codes_for(color, 3, own)
    st = Stage(color, vs, cc, sc, lit)
    fused = st.backward()
    views, counts = st.export()
    weights = _weights(color)
    grads, g_lat = functions.color_stage_weight_grads(color['eng'], color['cfg'], st.sv, st.ws_b, weights, want_latent=True)
    gates, seg, cnt = _gpu_gates(weights, st.sv['lat'], [v[0] for v in views])
    pts, up = np.concatenate([views[v][0] for v in seg]), np.concatenate([views[v][1] for v in seg])
    pick = lambda a: a if a.shape[0] == 1 else a[seg]
    _, _, ref_W, ref_b, ref_c, ref_s = ctr.gradients(color['Wc'], color['bc'], torch.from_numpy(pick(cc)), torch.from_numpy(pick(sc)), pts, cnt, up, gates)
    _assert_blocks('%s, %s codes, %d rows' % ('lit' if lit else 'unlit', 'own' if own else 'shared', len(pts)), grads, ref_W, ref_b)
    # the code gradients: rows of the views with points (float64: one row per segment for own codes, the sum for shared ones)
    lw = g_lat.double().cpu().numpy()
    fu = fused['g_lat'].astype(np.float64)
    assert not lw[1].any() and not fu[1].any()
    if own:
        ref_rows = np.concatenate([ref_s.numpy(), ref_c.numpy()], 1)
        for a, name in ((lw[seg], 'layer-wise'), (fu[seg], 'fused')):
            for blk in (slice(0, 256), slice(256, None)):
                assert np.abs(a[:, blk] - ref_rows[:, blk]).max() <= BAR * np.abs(ref_rows[:, blk]).max(), name
    else:
        ref_row = np.concatenate([ref_s.numpy(), ref_c.numpy()], 1)[0]
        for a, name in ((lw.sum(0), 'layer-wise'), (fu.sum(0), 'fused')):
            for blk in (slice(0, 256), slice(256, None)):
                assert np.abs(a[blk] - ref_row[blk]).max() <= BAR * np.abs(ref_row[blk]).max(), name


# ------------------------------------------------------------------------------------------------ 4, 5: additivity, determinism, chunks
def _autograd_run(color, vs, cc, sc, lit, with_weights):
    """forward + backward through color_stage_call with the loss sum(rgb * g_rgb) -> (rgb, [g_cc, g_sc, g_R, g_T, g_normal], weight
    gradients or None), numpy"""
    import torch
    from distr import functions
    req = lambda a: _t(a).requires_grad_(True)
    c, s, R, T, n = req(cc), req(sc), req(vs['R']), req(vs['T']), req(vs['normal'])
    weights = [w.requires_grad_(True) for w in _weights(color)] if with_weights else None
    kw = dict(normal=n, lights=_t(LIGHTS), energies=_t(ENERGIES)) if lit else {}
    rgb = functions.color_stage_call(color['eng'], color['cfg'], c, s, R, T, _t(vs['z']), _t(vs['mask'], np.uint8), weights=weights, **kw)
    (rgb * _t(vs['g_rgb'])).sum().backward()
    torch.cuda.synchronize()
    ins = [c, s, R, T] + ([n] if lit else [])
    return rgb.detach().cpu().numpy(), [t.grad.cpu().numpy() for t in ins], None if weights is None else [w.grad.cpu().numpy() for w in weights]


@pytest.mark.parametrize('lit', [False, True], ids=['unlit', 'lit'])
def test_additive_and_deterministic(color, lit):
    """With the weights on the node, rgb and the gradients to codes, cameras and the normal image are byte for byte those without; two
    runs with weights give the same eighteen gradients byte for byte."""
    vs = make_views([700, 0, 65], 38)
    cc, sc = codes_for(color, 3, True)
    off = _autograd_run(color, vs, cc, sc, lit, False)
    on = _autograd_run(color, vs, cc, sc, lit, True)
    again = _autograd_run(color, vs, cc, sc, lit, True)
    assert off[2] is None and len(on[2]) == 18 and len(off[1]) == (5 if lit else 4)
    for a, b in zip([off[0]] + off[1], [on[0]] + on[1]):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes() and np.abs(a).max() > 0
    for l, (a, b) in enumerate(zip(on[2], again[2])):
        assert np.isfinite(a).all() and np.abs(a).max() > 0 and a.tobytes() == b.tobytes(), l


def test_chunked_list(color, monkeypatch):
    """DISTR_TRAIN_MAX_BYTES so small that the lists of two views are cut into at least three train calls with a cut inside a view: the
    gradients are within 1e-4 of the uncut run's (another summation order) and byte-identical on a second run."""
    from distr import functions
    counts = [2049, 700]
    vs = make_views(counts, 39)
    cc, sc = codes_for(color, 2, True)
    whole = _autograd_run(color, vs, cc, sc, True, True)
    limit = functions.train_plan_bytes([512, 512], 3)
    plan = functions.render_train_chunks(counts, limit, out_dim=3)
    assert len(plan) >= 3 and any(a > 0 for piece in plan for _, a, _ in piece) and any(len(piece) > 1 for piece in plan), plan
    monkeypatch.setenv('DISTR_TRAIN_MAX_BYTES', str(limit))
    cut = _autograd_run(color, vs, cc, sc, True, True)
    again = _autograd_run(color, vs, cc, sc, True, True)
    for l, (a, b, c) in enumerate(zip(whole[2], cut[2], again[2])):
        assert b.tobytes() == c.tobytes(), l
    blocks = ctr.blockwise_residuals(cut[2], whole[2], CS)
    worst = max(blocks, key=lambda t: t[1])
    for a, b in zip([whole[0]] + whole[1], [cut[0]] + cut[1]):
        assert a.tobytes() == b.tobytes()
    print('lists of %r rows in %d pieces: worst block against the uncut run %s %.3e' % (counts, len(plan), worst[0], worst[1]))
    assert worst[1] <= BAR


# ------------------------------------------------------------------------------------------------ 6: the public path
def _renderers(fixture_decoder, weight_norm=False, **kw):
    import torch
    from core.sdfrenderer import SDFRenderer_color
    from distr import fixture
    from test_gpu_color_batch import _module
    Ws, bs, latent = fixture_decoder
    Wc, bc, code = fixture.make_color_decoder_weights(color_size=CS)
    dec = _module(Ws, bs, 256, [512] * 8, 1)
    dec_c = ctr.color_module(Wc, bc, weight_norm=weight_norm, dtype=torch.float32).cuda()
    r = SDFRenderer_color(dec, dec_c, fixture.make_intrinsic(48, 45), img_hw=(48, 45), march_step=30, buffer_size=2, **kw)
    return r, dec_c, np.asarray(latent, np.float32).reshape(1, 256), np.asarray(code, np.float32).reshape(1, CS)


def _cams():
    from distr import fixture
    cams = [fixture.make_camera(*c) for c in ((30.0, 20.0, 1.6, 10.0), (-75.0, -35.0, 1.9, 0.0))]
    return np.stack([c[0] for c in cams]).astype(np.float32), np.stack([c[1] for c in cams]).astype(np.float32)


@pytest.mark.parametrize('lit', [False, True], ids=['unlit', 'lit'])
def test_public_path_sgd_step_and_flag(fixture_decoder, lit):
    """SDFRenderer_color(color_decoder_grad=True).render_batch on the weight-norm colour module: every parameter of decoder_color gets a
    finite, non-zero gradient; with the flag off it gets none and every other byte, forward and backward, is the same. Then one SGD step:
    the next render_batch is byte for byte that of a fresh renderer on a module holding the updated state (the engine re-packs)."""
    import torch
    r, dec_c, latent, code = _renderers(fixture_decoder, weight_norm=True, color_decoder_grad=True)
    Rs, Ts = _cams()
    kw = dict(lighting_locations=_t(LIGHTS), lighting_energies=_t(ENERGIES)) if lit else {}
    w = _t(np.random.RandomState(40).standard_normal((2, 48, 45, 3)))

    def run():
        ins = [_t(a).requires_grad_(True) for a in (code, latent, Rs, Ts)]
        outs = r.render_batch(*ins, **kw)
        (outs[2] * w).sum().backward()
        return [o.detach().cpu().numpy() for o in outs], [t.grad.cpu().numpy() for t in ins]
    on = run()
    assert on[0][3].sum() > 200
    grads = {k: p.grad.clone() for k, p in dec_c.named_parameters()}
    assert len(grads) == 26 and all(torch.isfinite(g).all() and g.abs().max() > 0 for g in grads.values()), [k for k, g in grads.items() if not g.abs().max() > 0]
    for p in dec_c.parameters():
        p.grad = None
    r.color_decoder_grad = False
    off = run()
    assert all(p.grad is None for p in dec_c.parameters())
    for a, b in zip(on[0] + on[1], off[0] + off[1]):
        assert a.tobytes() == b.tobytes()
    # one SGD step on the gradients of the first backward
    r.color_decoder_grad = True
    for k, p in dec_c.named_parameters():
        p.grad = grads[k]
    with torch.no_grad():
        before = [o.cpu().numpy() for o in r.render_batch(_t(code), _t(latent), _t(Rs), _t(Ts), **kw)]
    torch.optim.SGD(dec_c.parameters(), lr=1e-3).step()
    with torch.no_grad():
        after = [o.cpu().numpy() for o in r.render_batch(_t(code), _t(latent), _t(Rs), _t(Ts), **kw)]
    fresh, twin, _, _ = _renderers(fixture_decoder, weight_norm=True)
    twin.load_state_dict(copy.deepcopy(dec_c.state_dict()))
    with torch.no_grad():
        want = [o.cpu().numpy() for o in fresh.render_batch(_t(code), _t(latent), _t(Rs), _t(Ts), **kw)]
    assert before[2].tobytes() != after[2].tobytes(), 'the step did not reach the packed colour engine'
    for a, b in zip(after, want):
        assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize('lit', [False, True], ids=['unlit', 'lit'])
def test_render_with_the_flag(fixture_decoder, lit):
    """render with the flag set: depth, normal, mask and min_sdf are the bytes of the flag-off call, the colours agree with it to the bound
    tests/test_gpu_color_batch.py uses between render_batch and render (p99 <= 1e-4 on the mask), and the colour decoder's parameters get
    gradients -- those of render_batch of the one view, byte for byte. Under no_grad (the argument or the context) the flag changes nothing."""
    import torch
    r, dec_c, latent, code = _renderers(fixture_decoder, color_decoder_grad=True)
    Rs, Ts = _cams()
    kw = dict(lighting_locations=_t(LIGHTS), lighting_energies=_t(ENERGIES)) if lit else {}
    w = _t(np.random.RandomState(41).standard_normal((48, 45, 3)))

    def run(batch=False, **more):
        for p in dec_c.parameters():
            p.grad = None
        ins = [_t(a).requires_grad_(True) for a in (code, latent, Rs[0], Ts[0])]
        if batch:
            outs = [o[0] for o in r.render_batch(ins[0], ins[1], ins[2][None], ins[3][None], **kw)]
        else:
            outs = r.render(*ins, **kw, **more)
        if outs[2].requires_grad:
            (outs[2] * w).sum().backward()
        return [o.detach().cpu().numpy() for o in outs], [None if p.grad is None else p.grad.cpu().numpy() for p in dec_c.parameters()]
    on, g_on = run()
    via_batch, g_batch = run(batch=True)
    r.color_decoder_grad = False
    off, g_off = run()
    assert all(g is None for g in g_off) and all(g is not None and np.abs(g).max() > 0 for g in g_on)
    for i in (0, 1, 3, 4):
        assert on[i].shape == off[i].shape and on[i].tobytes() == off[i].tobytes(), i
    m = off[3].astype(bool)
    assert m.sum() > 200 and on[2].shape == off[2].shape and not on[2][~m].any()
    assert np.percentile(np.abs(on[2] - off[2])[m], 99) <= 1e-4
    for a, b in zip(on + g_on, via_batch + g_batch):
        assert a.tobytes() == b.tobytes()
    no_grad_off = run(no_grad=True)[0]
    r.color_decoder_grad = True
    no_grad_on, g = run(no_grad=True)
    assert all(x is None for x in g)
    for a, b in zip(no_grad_on, no_grad_off):
        assert a.tobytes() == b.tobytes()
    with torch.no_grad():
        a = r.render(_t(code), _t(latent), _t(Rs[0]), _t(Ts[0]), **kw)
        r.color_decoder_grad = False
        b = r.render(_t(code), _t(latent), _t(Rs[0]), _t(Ts[0]), **kw)
    for x, y in zip(a, b):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()


def test_refusals(fixture_decoder):
    import torch
    from distr import decoder_pack
    Rs, Ts = _cams()
    r, dec_c, latent, code = _renderers(fixture_decoder, color_decoder_grad=True)
    ins = lambda: [_t(a).requires_grad_(True) for a in (code, latent, Rs, Ts)]
    with pytest.raises(ValueError, match='lighting_locations requires grad'):
        r.render_batch(*ins(), lighting_locations=_t(LIGHTS).requires_grad_(True))
    with pytest.raises(ValueError, match='lighting_energies requires grad'):
        r.render_batch(*ins(), lighting_locations=_t(LIGHTS), lighting_energies=_t(ENERGIES).requires_grad_(True))
    # nothing to do: no parameter of decoder_color requires grad -- taken, and the flag changes nothing
    for p in dec_c.parameters():
        p.requires_grad_(False)
    out = r.render_batch(*ins())
    out[2].sum().backward()
    assert all(p.grad is None for p in dec_c.parameters())
    # a colour decoder in training mode with dropout raises as everywhere
    from distr import fixture
    from core.sdfrenderer import SDFRenderer_color
    Wc, bc, _ = fixture.make_color_decoder_weights(color_size=CS)
    drop = ctr.color_module(Wc, bc, dropout=list(range(8)), dropout_prob=0.2, dtype=torch.float32).cuda()
    r2 = SDFRenderer_color(r.decoder, drop, fixture.make_intrinsic(48, 45), img_hw=(48, 45), march_step=30, buffer_size=2, color_decoder_grad=True)
    drop.train()
    with pytest.raises(decoder_pack.UnsupportedDecoder, match='training mode'):
        r2.render_batch(*ins())
    with pytest.raises(decoder_pack.UnsupportedDecoder, match='training mode'):
        r2.render(*[t[0] if t.shape[0] == 2 else t for t in ins()])
    # weights together with detach_color
    from distr import functions
    vs = make_views([65], 42)
    weights = [_t(a).requires_grad_(True) for a in list(Wc) + list(bc)]
    with pytest.raises(ValueError, match='detach_color'):
        functions.color_stage_call(r._color_engine, _cfg48(), _t(code), _t(latent), _t(vs['R']).requires_grad_(True), _t(vs['T']), _t(vs['z']),
                                   _t(vs['mask'], np.uint8), normal=_t(vs['normal']), lights=_t(LIGHTS), detach_color=True, weights=weights)
    # weights of another colour decoder
    W64, b64, _ = fixture.make_color_decoder_weights(color_size=64)
    other = [_t(a).requires_grad_(True) for a in list(W64) + list(b64)]
    rgb = functions.color_stage_call(r._color_engine, _cfg48(), _t(code), _t(latent), _t(vs['R']), _t(vs['T']), _t(vs['z']), _t(vs['mask'], np.uint8), weights=other)
    with pytest.raises(ValueError, match='code length 320'):
        rgb.sum().backward()


def _cfg48():
    from distr import binding, fixture
    return binding.make_cfg((H, W), fixture.make_intrinsic(H, W), marcher='recursive')


# ------------------------------------------------------------------------------------------------ 7: the public path against the reference
@pytest.mark.parametrize('case', ['unlit', 'lit', 'wn'])
def test_public_path_against_g35(fixture_decoder, case):
    """SDFRenderer_color(color_decoder_grad=True).render + compute_loss_color(use_ssim=True) + backward on G35's scene: the mask equals
    the reference's, and rgb, both loss values and the gradients of both codes, R, T and every recorded quantity of the colour decoder's
    parameters (for `wn`: weight_g, the digests of weight_v) are inside max(1e-3, 2 x the reference's own floor) -- the host bars."""
    import os
    import torch
    from conftest import GOLDEN
    from core.sdfrenderer import SDFRenderer_color
    from core.utils.loss_utils import compute_loss_color
    from distr import fixture
    from test_gpu_color_batch import _module
    import color_render_train_restatement as crt
    import render_train_restatement as rt
    g = dict(np.load(os.path.join(GOLDEN, 'g35_color_render_weight_grad.npz')))
    lit, wn = crt.CASES[case]
    Ws, bs, _ = fixture_decoder
    Wc, bc, _ = fixture.make_color_decoder_weights(color_size=int(g['color_size']))
    dec_c = ctr.color_module(Wc, bc, weight_norm=wn, dtype=torch.float32)
    if wn:
        dec_c.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in crt.wn_state_dict(g, Wc, bc).items()})
    dec_c = dec_c.cuda()
    r = SDFRenderer_color(_module(Ws, bs, 256, [512] * 8, 1), dec_c, g['K'], img_hw=(int(g['H']), int(g['W'])), march_step=int(g['march_step']),
                          buffer_size=int(g['buffer_size']), color_decoder_grad=True)
    cc, lat, R, T = (_t(g[k]).requires_grad_(True) for k in ('color_code', 'latent', 'R', 'T'))
    kw = dict(lighting_locations=_t(g['lights']), lighting_energies=_t(g['energies'])) if lit else {}
    _, _, rgb, mask, _ = r.render(cc, lat, R, T, **kw)
    assert int((mask.cpu().numpy() != g[case + '_mask']).sum()) == 0
    img = rgb.detach().cpu().numpy()
    l1, ssim, _ = compute_loss_color(rgb, mask, _t(g[case + '_gt']), _t(g['gt_mask'], np.uint8), use_ssim=True)
    (l1 + ssim).backward()
    params = dict(dec_c.named_parameters())
    gp = lambda n: params[n].grad.detach().cpu().numpy()
    gb = [gp('lin%d.bias' % l) for l in range(9)]
    if wn:
        got = rt.recorded([None] * 8 + [gp('lin8.weight')], gb, [gp('lin%d.weight_g' % l) for l in range(8)], [gp('lin%d.weight_v' % l) for l in range(8)])
    else:
        got = rt.recorded([gp('lin%d.weight' % l) for l in range(9)], gb)
    got.update(g_color_code=cc.grad.cpu().numpy(), g_latent=lat.grad.cpu().numpy(), g_R=R.grad.cpu().numpy(), g_T=T.grad.cpu().numpy(), rgb=img,
               l1=l1.item(), ssim=ssim.item())
    res = crt.residuals(got, g, case)
    worst = max(res, key=lambda t: t[1] / t[2])
    print('public path against G35 %s: %d quantities, worst against its bar %s %.1e (bar %.1e)' % ((case, len(res)) + worst))
    bad = [(k, v, bar) for k, v, bar in res if not v <= bar]
    assert not bad, bad
