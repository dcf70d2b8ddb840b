"""Weight gradients through render on the GPU: the export of the backward's sample list
(distr_render_samples_export_batch), the layer-wise train path run over it (functions.render_weight_grads, the optional trailing weights of
RenderBatchFunction) and SDFRenderer(decoder_grad=True).

Expected values never come from the code under test, except where a test says so: the lists are the CPU oracle's
(RenderState.samples), the weight gradients tests/train_restatement.gradients in float64 over the oracle's list on the ReLU gates the GPU
saved, the public path's gradients the reference's own (golden G33). Scenes are 48 x 40 (and the 32 x 32 pad scene of
tests/test_gpu_bwd_list.py); every oracle render, GPU forward and float64 gradient is made once per module and not modified."""
import copy
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN

import render_train_restatement as rt
import train_restatement as tr

pytestmark = pytest.mark.gpu

GUARD = 4096
BAR = 1e-4              # the project's bar for another f32 summation order, of a tensor's (block's) largest entry
KEYS = ('g_zdepth', 'g_min_sdf', 'g_depth', 'g_normal')


@pytest.fixture(scope='module')
def g33():
    return dict(np.load(os.path.join(GOLDEN, 'g33_render_weight_grad.npz')))


# ------------------------------------------------------------------------------------------------ the GPU side
def _guarded(nbytes, dev):
    import torch
    buf = torch.empty(nbytes + 2 * GUARD, dtype=torch.uint8, device=dev)
    buf[:GUARD] = 0xA5
    buf[GUARD:GUARD + nbytes] = 0xFF
    buf[GUARD + nbytes:] = 0xA5
    return buf


def _whole(buf, nbytes):
    return bool((buf[:GUARD] == 0xA5).all()) and bool((buf[GUARD + nbytes:] == 0xA5).all())


class Rendered(object):
    """One render_batch_call of B views with codes and cameras that require grad; backward(ups) calls distr_render_backward_batch on the
    saved forward workspace as RenderBatchFunction.backward does; export() calls distr_render_samples_export_batch into arrays that lie
    between 0xA5 guards and are pre-filled with 0xFF."""

    def __init__(self, eng, H, W, K, kw, lat, Rs, Ts):
        import torch
        from distr import binding, functions
        dev = eng.device
        self.eng, self.B, self.P = eng, len(Rs), H * W
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev).requires_grad_(True)
        self.lat = t(lat)
        self.out = functions.render_batch_call(eng, binding.make_cfg((H, W), K, arith='f32', **kw), self.lat, t(np.stack(Rs)), t(np.stack(Ts)))
        self.node = self.out[2].grad_fn
        self.cfg, self.ws = self.node.cfg, self.node.ws
        self.ws_b = torch.empty(self.B * eng.ctx.workspace_bytes(self.cfg)[1], dtype=torch.uint8, device=dev)

    def backward(self, ups):
        """ups: per view a dict of upstream gradients (KEYS; a missing one is zero for that view) -> (g_latent, g_R, g_T) numpy."""
        import torch
        from distr import binding
        eng, B, P = self.eng, self.B, self.P
        dev = eng.device
        self.ws_b.fill_(0xFF)
        g = []
        for k in KEYS:
            n = 3 * P if k == 'g_normal' else P
            if not any(k in u for u in ups) or (k in ('g_depth', 'g_normal') and not self.cfg.want_normal):
                g.append(None)
                continue
            g.append(torch.from_numpy(np.stack([np.asarray(u.get(k, np.zeros(n)), np.float32).reshape(n) for u in ups])).to(dev).contiguous())
        nan = lambda *s: torch.full(s, float('nan'), dtype=torch.float32, device=dev)
        g_lat, g_R, g_T = nan(B, eng.latent_size), nan(B, 9), nan(B, 3)
        p = binding.ptr
        eng.ctx.check(eng.ctx.L.distr_render_backward_batch(eng.ctx.h, C.byref(self.cfg), B, p(self.ws), self.ws.numel(), p(g[0]), p(g[1]), p(g[2]), p(g[3]),
                                                            p(g_lat), p(g_R), p(g_T), p(self.ws_b), self.ws_b.numel(), eng.ctx.stream()))
        torch.cuda.synchronize()
        return g_lat.cpu().numpy(), g_R.cpu().numpy(), g_T.cpu().numpy()

    def export(self):
        """-> per view (xyz (n, 3) f32, coef (n,) f32, src (n,) int32). Asserts whole guards, untouched rows behind every count, and that a
        call without src writes the same xyz / coef bytes."""
        import torch
        eng, B = self.eng, self.B
        L = eng.ctx.L
        cap = int(L.distr_render_max_samples(C.byref(self.cfg)))
        assert cap == self.P * self.cfg.buffer_size + 1
        sizes = dict(xyz=B * cap * 12, coef=B * cap * 4, src=B * cap * 4, counts=B * 4)
        bufs = {k: _guarded(n, eng.device) for k, n in sizes.items()}
        at = lambda k: C.c_void_p(bufs[k].data_ptr() + GUARD)
        eng.ctx.check(L.distr_render_samples_export_batch(eng.ctx.h, C.byref(self.cfg), B, C.c_void_p(self.ws.data_ptr()), self.ws.numel(),
                                                          C.c_void_p(self.ws_b.data_ptr()), self.ws_b.numel(), at('xyz'), at('coef'), at('src'), cap, at('counts'),
                                                          eng.ctx.stream()))
        torch.cuda.synchronize()
        for k, n in sizes.items():
            assert _whole(bufs[k], n), 'a guard of the %s array was written' % k
        raw = {k: bufs[k][GUARD:GUARD + n].cpu().numpy() for k, n in sizes.items()}
        counts = raw['counts'].view(np.int32)
        assert (counts >= 0).all() and (counts <= cap).all(), counts
        xyz, coef, src = raw['xyz'].reshape(B, cap * 12), raw['coef'].reshape(B, cap * 4), raw['src'].reshape(B, cap * 4)
        views = []
        for v in range(B):
            n = int(counts[v])
            assert (xyz[v, n * 12:] == 0xFF).all() and (coef[v, n * 4:] == 0xFF).all() and (src[v, n * 4:] == 0xFF).all(), 'rows at or beyond the count were written'
            views.append((xyz[v, :n * 12].view(np.float32).reshape(n, 3).copy(), coef[v, :n * 4].view(np.float32).copy(), src[v, :n * 4].view(np.int32).copy()))
        from distr import functions
        x2, c2, s2, n2 = functions.render_samples(eng, self.cfg, self.ws, self.ws_b, B)               # the Python entry, without src
        assert s2 is None and np.array_equal(n2.cpu().numpy(), counts)
        for v in range(B):
            n = int(counts[v])
            assert np.array_equal(x2[v, :n].cpu().numpy().view(np.uint32), views[v][0].view(np.uint32)) and np.array_equal(c2[v, :n].cpu().numpy().view(np.uint32), views[v][1].view(np.uint32))
        return views


def canon(pts, coef):
    """The canonical order of a list: by the points' bit patterns, then by the coefficient."""
    b = np.ascontiguousarray(pts, np.float32).view(np.uint32).reshape(-1, 3)
    return np.lexsort((np.asarray(coef, np.float32), b[:, 2], b[:, 1], b[:, 0]))


def ulps(a, b):
    """Distance of two f32 arrays in units of the last place (same sign assumed where it matters; the bit patterns as integers)."""
    ia, ib = np.asarray(a, np.float32).view(np.int32).astype(np.int64), np.asarray(b, np.float32).view(np.int32).astype(np.int64)
    return np.abs(ia - ib)


# ------------------------------------------------------------------------------------------------ scenes: the oracle's lists
@pytest.fixture(scope='module')
def scenes(g33, cpu_oracle, orc, fixture_decoder):
    """name -> dict(H, W, K, R, T, latent, kw, up: the upstream gradients, list: the oracle's (pix, pts, coef), d2n: normals from depth
    feed the coefficients). The two G33 scenes, the pad scene of test_gpu_bwd_list.py (the list ends in the combined pad sample), and the
    G33 camera with buffer_size = 8 on the pyramid (the selected rows of short rays include coarse-level rows)."""
    from test_gpu_bwd_list import KW_C, _pad_case
    Ws, bs, latent = fixture_decoder
    H, W, seed = int(g33['H']), int(g33['W']), int(g33['loss_seed'])
    out = {}

    def add(name, kw, kind, seed_):
        o = cpu_oracle.render(orc.make_cfg(H, W, g33['K'], **kw), latent, g33['R'], g33['T'])
        up = rt.upstream(kind, H, W, seed_, o['mask'])
        out[name] = dict(H=H, W=W, K=g33['K'], R=g33['R'], T=g33['T'], latent=latent, kw=kw, up=up, list=o['state'].samples(**up), d2n=kind == 'render',
                         state=o['state'])
    add('pyr_d2n', rt.cfg_kw(g33, 'pyr_d2n'), 'render', seed)
    add('rec_depth', rt.cfg_kw(g33, 'rec_depth'), 'render_depth', seed)
    add('coarse', dict(marcher='pyramid_recursive', march_step=int(g33['march_step']), buffer_size=8, want_normal=False), 'render_depth', seed + 1)
    c, gz, gq, lst = _pad_case(cpu_oracle, orc, fixture_decoder, 32, 64)
    out['pad'] = dict(H=32, W=32, K=c['K'], R=c['R'], T=c['T'], latent=latent, kw=dict(KW_C), up=dict(g_zdepth=gz, g_min_sdf=gq), list=lst, d2n=False, state=c['state'])
    assert len(out['pyr_d2n']['list'][0]) == int(g33['pyr_d2n_num_samples']) and len(out['rec_depth']['list'][0]) == int(g33['rec_depth_num_samples'])
    return out


@pytest.fixture(scope='module')
def rendered(engine, scenes):
    """name -> (Rendered of the scene alone after its backward, its exported list)"""
    out = {}
    for name, s in scenes.items():
        r = Rendered(engine, s['H'], s['W'], s['K'], s['kw'], s['latent'], [s['R']], [s['T']])
        r.grads = r.backward([s['up']])
        out[name] = (r, r.export()[0])
    return out


# ------------------------------------------------------------------------------------------------ 1: the export against the oracle
@pytest.mark.parametrize('name', ['pyr_d2n', 'rec_depth', 'pad', 'coarse'])
def test_export_matches_the_oracle(scenes, rendered, name):
    """After a canonical sort the exported points equal RenderState.samples() bit for bit and the counts are equal. The coefficients:
    bit for bit where a single upstream term flows into the sample (ratio * g_zdepth: one f32 product, correctly rounded on both sides; or
    g_min_sdf alone); where g_zdepth and g_min_sdf ADD in a row (the row k = 0 of a hit pixel) the oracle rounds ratio * gz + gq once from
    double and the kernel rounds the product and the sum in f32: at most one unit in the last place apart (both terms positive here); the
    combined pad sample sums its rows in another order and precision: n rows, each rounding <= 2^-24 of the running sum, all one sign:
    n * 2^-23 of the coefficient. With depth2normal upstream (five stencil terms, reassociated): 1e-5 of the view's largest |coef|."""
    s = scenes[name]
    pix, pts, coef = s['list']
    xyz, cf, src = rendered[name][1]
    assert len(cf) == len(coef), (name, 'counts', len(cf), len(coef))
    a, b = canon(xyz, cf), canon(pts, coef)
    assert np.array_equal(xyz[a].view(np.uint32), pts[b].view(np.uint32)), (name, 'points differ', int((xyz[a].view(np.uint32) != pts[b].view(np.uint32)).any(1).sum()))
    ga, gb = cf[a], coef[b]
    n_pad = int((src < 0).sum())
    assert n_pad == int((pix < 0).sum()) and (n_pad == 0 or (src[-1] == -1 and not xyz[-1].any()))       # the pad sample comes last, at the origin
    if name == 'pad':
        assert n_pad == 1
    if name == 'coarse':
        lv = src[src >= 0] >> 28
        assert (lv == 0).any() and (lv > 0).any(), 'the list should hold full-resolution and coarse-level rows'
        print('coarse scene: %d full-resolution rows, %d coarse rows' % (int((lv == 0).sum()), int((lv > 0).sum())))
    diff = ga.view(np.uint32) != gb.view(np.uint32)
    print('%s: %d samples, %d pad; coefficients not bit-identical: %d, largest distance %d ulp, %.3e of the largest |coef|'
          % (name, len(cf), n_pad, int(diff.sum()), int(ulps(ga, gb).max()), float(np.abs(ga.astype(np.float64) - gb).max() / np.abs(gb).max())))
    if s['d2n']:
        assert np.abs(ga.astype(np.float64) - gb).max() <= 1e-5 * np.abs(gb).max()
        return
    # which samples carry one term, which the sum of two: from the upstream gradients and the oracle's own list (pixel, row order)
    gz, gq = s['up']['g_zdepth'], s['up']['g_min_sdf']
    px = pix[b]
    first = np.zeros(len(pix), bool)                       # the oracle lists a pixel's rows k = 0, 1, .. in order: its first entry is row k = 0 if that row is listed
    seen = set()
    for i, p_ in enumerate(pix):
        if p_ >= 0 and p_ not in seen:
            seen.add(int(p_))
            first[i] = True
    two = np.zeros(len(pix), bool)
    real = pix >= 0
    two[real] = first[real] & (gz[pix[real]] != 0) & (gq[pix[real]] != 0)
    two = two[b]
    pad = px < 0
    one = ~two & ~pad
    assert not diff[one].any(), (name, 'single-term coefficients differ', int(diff[one].sum()))
    assert (ulps(ga[two], gb[two]) <= 1).all(), (name, 'two-term coefficients', int(ulps(ga[two], gb[two]).max()))
    if pad.any():
        npad_rows = int((gz != 0).sum()) * s['kw']['buffer_size']      # an upper bound of the padded rows that carry a coefficient
        assert abs(float(ga[pad][0]) - float(gb[pad][0])) <= npad_rows * 2.0 ** -23 * abs(float(gb[pad][0])) and ga[pad][0] != 0


# ------------------------------------------------------------------------------------------------ 2: the views of a batch
@pytest.mark.parametrize('codes', ['shared', 'own'])
def test_batch_views_equal_their_own_call(engine, scenes, fixture_decoder, codes):
    """B = 4 with counts that differ; view 2 has an all-zero upstream gradient (count 0). Every view's exported rows are, byte for byte,
    those of its own B = 1 call (expected values from the code under test: this is a consistency check of the batch form)."""
    from distr import fixture
    s = scenes['rec_depth']
    H, W, P = s['H'], s['W'], s['H'] * s['W']
    cams = [(s['R'], s['T'])] + [fixture.make_camera(*c) for c in ((20, 10, 1.6, 0), (-35, 18, 1.6, 8), (60, -10, 1.8, 3))]
    rs = np.random.RandomState(41)
    lat = s['latent'] if codes == 'shared' else (s['latent'] + 0.1 * np.abs(s['latent']).max() * rs.standard_normal((4, s['latent'].shape[1]))).astype(np.float32)
    ups = []
    for v in range(4):
        gz, gq = rs.rand(P).astype(np.float32), rs.rand(P).astype(np.float32)
        if v == 2:
            gz[:], gq[:] = 0, 0
        if v == 3:
            gq[:] = 0                      # fewer samples: only the hit pixels
        ups.append(dict(g_zdepth=gz, g_min_sdf=gq))
    batch = Rendered(engine, H, W, s['K'], s['kw'], lat, [c[0] for c in cams], [c[1] for c in cams])
    gb = batch.backward(ups)
    got = batch.export()
    counts = [len(g[1]) for g in got]
    assert counts[2] == 0 and len(set(counts)) == 4, counts
    for v in range(4):
        alone = Rendered(engine, H, W, s['K'], s['kw'], lat if codes == 'shared' else lat[v:v + 1], [cams[v][0]], [cams[v][1]])
        ga = alone.backward([ups[v]])
        exp = alone.export()[0]
        for name, a, b in zip(('xyz', 'coef', 'src'), got[v], exp):
            assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32)), (codes, v, name)
        for name, a, b in zip(('g_latent', 'g_R', 'g_T'), gb, ga):
            assert np.array_equal(a[v], b[0]), (codes, v, name)
    print('batch (%s codes): counts %r' % (codes, counts))


# ------------------------------------------------------------------------------------------------ 3: the weight gradients
def _weights(Ws, bs):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda() for a in list(Ws) + list(bs)]


def _gpu_gates(weights, lat, pts):
    """The ReLU pattern the train path saves for the list `pts` (one segment), eight boolean tensors in list order."""
    import torch
    from distr import functions
    n = len(pts)
    _, saved = functions.train_forward(weights, lat, torch.from_numpy(np.ascontiguousarray(pts, np.float32)).cuda(), [n])
    return [(saved.activations(l + 1)[:n] > 0).cpu() for l in range(8)]


def _assert_weight_grads(tag, got, ref_W, ref_b, Cn):
    res = []
    for i, (a, b) in enumerate(zip(got, list(ref_W) + list(ref_b))):
        a, b = a.double().cpu(), b.double().reshape(a.shape)
        res.append(((a - b).abs().max() / b.abs().max()).item())
    blocks = tr.blockwise_residuals([g.cpu() for g in got], list(ref_W) + list(ref_b), Cn)
    worst = max(blocks, key=lambda t: t[1])
    print('%s: largest residual of a tensor %.3e (g_%s%d), of a block %.3e (%s)' % (tag, max(res), 'Wb'[int(np.argmax(res)) // 9], int(np.argmax(res)) % 9, worst[1], worst[0]))
    assert max(res) <= BAR, (tag, res)
    assert worst[1] <= BAR, (tag, worst)
    return max(max(res), worst[1])


@pytest.mark.parametrize('name', ['pyr_d2n', 'rec_depth'])
def test_weight_gradients_match_float64_on_the_oracles_list(engine, scenes, rendered, fixture_decoder, name):
    """render_weight_grads on the workspaces of the scene's backward against float64 gradients over the ORACLE's list, every ReLU on the
    gate the train path saved at that point (the GPU's list holds the same points: its rows are matched to the oracle's by the canonical
    order). 1e-4 of each tensor's largest entry, and per block."""
    import torch
    from distr import functions
    Ws, bs, latent = fixture_decoder
    s, (r, (xyz, cf, src)) = scenes[name], rendered[name]
    pix, pts, coef = s['list']
    weights = _weights(Ws, bs)
    grads, g_lat = functions.render_weight_grads(engine, r.cfg, r.ws, r.ws_b, 1, weights, r.lat)
    gates_gpu = _gpu_gates(weights, r.lat.detach(), xyz)
    a, b = canon(xyz, cf), canon(pts, coef)
    inv = np.empty(len(b), np.int64)
    inv[b] = a                                              # oracle row i is the GPU's row inv[i]
    gates = [g[torch.from_numpy(inv)] for g in gates_gpu]
    _, _, ref_W, ref_b, ref_c = tr.gradients(Ws, bs, latent, pts, [len(pts)], coef, None, gates)
    _assert_weight_grads('%s (%d samples)' % (name, len(pts)), grads, ref_W, ref_b, 256)
    # the layer-wise code gradient against float64, and against the fused backward's
    rel64 = ((g_lat.double().cpu() - ref_c).abs().max() / ref_c.abs().max()).item()
    fused = torch.from_numpy(r.grads[0]).double()
    rel_fused = ((g_lat.double().cpu() - fused).abs().max() / fused.abs().max()).item()
    print('%s: layer-wise g_latent %.3e from float64, %.3e from the fused backward' % (name, rel64, rel_fused))
    assert rel64 <= BAR and rel_fused <= BAR


@pytest.mark.parametrize('Cn', [64, 300])
def test_weight_gradients_other_code_lengths(Cn):
    """Code lengths 64 and 300. The oracle is built for C = 256 only, so here the list is the GPU's OWN export (pinned against the oracle
    at C = 256 above); the expected gradients are float64 over that list on the gates the train path saved."""
    import torch
    from distr import fixture, functions
    Ws, bs, latent = fixture.make_decoder_weights(latent_size=Cn)
    eng = functions.engine_from_weights(Ws, bs, 0)
    H, W = 48, 40
    K = np.array([[44.0, 0.0, 20.0], [0.0, 46.0, 24.0], [0.0, 0.0, 1.0]])
    R, T = fixture.make_camera(-50, 25, 1.7, 4)
    r = Rendered(eng, H, W, K, dict(marcher='pyramid_recursive', march_step=24, buffer_size=3, use_depth2normal=True), latent, [R], [T])
    mask = r.out[1].cpu().numpy().reshape(H, W)
    assert mask.sum() > 100
    r.backward([rt.upstream('render', H, W, 5, mask)])
    xyz, cf, src = r.export()[0]
    assert len(cf) > 1000
    weights = _weights(Ws, bs)
    grads, g_lat = functions.render_weight_grads(eng, r.cfg, r.ws, r.ws_b, 1, weights, r.lat)
    _, _, ref_W, ref_b, ref_c = tr.gradients(Ws, bs, latent, xyz, [len(xyz)], cf, None, _gpu_gates(weights, r.lat.detach(), xyz))
    _assert_weight_grads('C = %d (%d samples)' % (Cn, len(cf)), grads, ref_W, ref_b, Cn)
    assert ((g_lat.double().cpu() - ref_c).abs().max() / ref_c.abs().max()).item() <= BAR


# ------------------------------------------------------------------------------------------------ 4, 5: additivity, determinism, chunks
def _autograd_run(engine, s, Ws, bs, with_weights, B=1, kw=None):
    """One forward + backward through the render node with the scene's seeded loss -> (outputs, (g_latent, g_R, g_T), weight gradients or None), numpy."""
    import torch
    from distr import binding, functions
    import helpers
    dev = engine.device
    H, W = s['H'], s['W']
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev).requires_grad_(True)
    lat, Rt, Tt = t(s['latent']), t(np.stack([s['R']] * B)), t(np.stack([s['T']] * B))
    weights = [w.requires_grad_(True) for w in _weights(Ws, bs)] if with_weights else None
    out = functions.render_batch_call(engine, binding.make_cfg((H, W), s['K'], **(kw or s['kw'])), lat, Rt, Tt, weights=weights)
    z, m, q, depth, normal = out
    wd, wq, wn = (torch.from_numpy(a).to(dev) for a in helpers.loss_weights(H, W, 5))
    mb = m.reshape(B, H, W).bool()
    if s['d2n']:
        L = (depth * wd)[mb].sum() + (q.reshape(B, H, W) * wq).sum() + (normal * wn).sum()
    else:
        L = (z.reshape(B, H, W) * wd)[mb].sum() + (q.reshape(B, H, W) * wq).sum()
    L.backward()
    torch.cuda.synchronize()
    outs = [o.detach().cpu().numpy() for o in out]
    return outs, [g.grad.cpu().numpy() for g in (lat, Rt, Tt)], None if weights is None else [w.grad.cpu().numpy() for w in weights]


@pytest.mark.parametrize('name', ['pyr_d2n', 'rec_depth'])
def test_additive_and_deterministic(engine, scenes, fixture_decoder, name):
    """With the weights on the node, the forward outputs and g_latent / g_R / g_T are byte for byte those without; two runs with weights
    give the same eighteen gradients byte for byte."""
    Ws, bs, _ = fixture_decoder
    s = scenes[name]
    off = _autograd_run(engine, s, Ws, bs, False)
    on = _autograd_run(engine, s, Ws, bs, True)
    again = _autograd_run(engine, s, Ws, bs, True)
    assert off[2] is None and len(on[2]) == 18
    for a, b in zip(off[0] + off[1], on[0] + on[1]):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    for l, (a, b) in enumerate(zip(on[2], again[2])):
        assert np.isfinite(a).all() and np.abs(a).max() > 0 and a.tobytes() == b.tobytes(), l


def test_chunked_list(engine, scenes, fixture_decoder, monkeypatch):
    """DISTR_TRAIN_MAX_BYTES so small that the list of two views is cut into at least three train calls with one cut inside a view: the
    gradients are within 1e-4 of the uncut run's (another summation order) and byte-identical on a second run."""
    from distr import functions
    Ws, bs, _ = fixture_decoder
    s = scenes['rec_depth']
    whole = _autograd_run(engine, s, Ws, bs, True, B=2)
    n = len(s['list'][0])
    limit = functions.train_plan_bytes([1024, 1024])
    plan = functions.render_train_chunks([n, n], limit)
    assert len(plan) >= 3 and any(a > 0 for piece in plan for _, a, _ in piece) and any(len(piece) > 1 for piece in plan), plan
    monkeypatch.setenv('DISTR_TRAIN_MAX_BYTES', str(limit))
    cut = _autograd_run(engine, s, Ws, bs, True, B=2)
    again = _autograd_run(engine, s, Ws, bs, True, B=2)
    worst = 0.0
    for l, (a, b, c) in enumerate(zip(whole[2], cut[2], again[2])):
        assert b.tobytes() == c.tobytes(), l
        worst = max(worst, float(np.abs(a.astype(np.float64) - b).max() / np.abs(a).max()))
    for a, b in zip(whole[0] + whole[1], cut[0] + cut[1]):
        assert a.tobytes() == b.tobytes()
    print('list of 2 x %d samples in %d pieces %r: largest distance from the uncut run %.3e' % (n, len(plan), [[(v, a, k) for v, a, k in p] for p in plan], worst))
    assert worst <= BAR


# ------------------------------------------------------------------------------------------------ 6: the public path
def _wn_module(g33, fixture_decoder, **kw):
    import torch
    from core.graph.deep_sdf_decoder import Decoder
    Ws, bs, _ = fixture_decoder
    dec = Decoder(256, [512] * 8, norm_layers=tuple(range(8)), latent_in=[4], weight_norm=True, **kw)
    dec.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in rt.wn_state_dict(g33, Ws, bs).items()})
    return dec.cuda().eval()


def _public_render(r, g33, no_grad=False):
    import torch
    import helpers
    H, W = int(g33['H']), int(g33['W'])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda().requires_grad_(not no_grad)
    lat, R, T = t(g33['latent']), t(g33['R']), t(g33['T'])
    depth, normal, mask, q = r.render(lat, R, T, no_grad=no_grad)
    wd, wq, wn = (torch.from_numpy(a).cuda() for a in helpers.loss_weights(H, W, int(g33['loss_seed'])))
    L = (depth * wd)[mask.bool()].sum() + (q * wq).sum() + (normal * wn).sum()
    return (depth, normal, mask, q), L, (lat, R, T)


def test_public_path_weight_norm_and_sgd_step(g33, fixture_decoder):
    """SDFRenderer(decoder_grad=True).render on the weight-norm module: the gradients of weight_g, weight_v, lin8.weight, the biases, the code
    and the camera against the reference's own (G33 `wn`), every recorded quantity at max(1e-3, 2 x its floor). Then one SGD step on the
    decoder: the next render is byte for byte that of a fresh renderer built on a copy of the updated module (the engine re-packs)."""
    import torch
    from core.sdfrenderer import SDFRenderer
    dec = _wn_module(g33, fixture_decoder)
    kw = dict(img_hw=(int(g33['H']), int(g33['W'])), march_step=int(g33['march_step']), buffer_size=int(g33['buffer_size']), use_depth2normal=True)
    r = SDFRenderer(dec, g33['K'], decoder_grad=True, **kw)
    outs, L, (lat, R, T) = _public_render(r, g33)
    assert int((outs[2].cpu().numpy().astype(np.uint8) != g33['wn_mask']).sum()) <= 1
    L.backward()
    params = dict(dec.named_parameters())
    g = lambda n: params[n].grad.detach().cpu().numpy()
    got = rt.recorded([None] * 8 + [g('lin8.weight')], [g('lin%d.bias' % l) for l in range(9)], [g('lin%d.weight_g' % l) for l in range(8)],
                      [g('lin%d.weight_v' % l) for l in range(8)])
    got.update(g_latent=lat.grad.cpu().numpy(), g_R=R.grad.cpu().numpy(), g_T=T.grad.cpu().numpy())
    res = rt.residuals(got, g33, 'wn')
    print('public path against G33 wn:', ', '.join('%s %.1e' % (k, v) for k, v, _ in res))
    bad = [(k, v, bar) for k, v, bar in res if not v <= bar]
    assert not bad, bad
    # with the flag off the decoder gets no gradient and the codes' and cameras' are the same bytes
    for p in dec.parameters():
        p.grad = None
    r.decoder_grad = False
    _, L0, (lat0, R0, T0) = _public_render(r, g33)
    L0.backward()
    assert all(p.grad is None for p in dec.parameters())
    for a, b in ((lat0, lat), (R0, R), (T0, T)):
        assert a.grad.cpu().numpy().tobytes() == b.grad.cpu().numpy().tobytes()
    # one SGD step (on the gradients of the first backward)
    r.decoder_grad = True
    before = [o.detach().cpu().numpy() for o in _public_render(r, g33, no_grad=True)[0]]
    _, L1, _ = _public_render(r, g33)
    L1.backward()
    torch.optim.SGD(dec.parameters(), lr=1e-6).step()
    after = [o.detach().cpu().numpy() for o in _public_render(r, g33, no_grad=True)[0]]
    twin = _wn_module(g33, fixture_decoder)                   # (a weight-norm module that has run cannot be deep-copied: a new one, the same state)
    twin.load_state_dict(copy.deepcopy(dec.state_dict()))
    fresh = SDFRenderer(twin, g33['K'], **kw)
    want = [o.detach().cpu().numpy() for o in _public_render(fresh, g33, no_grad=True)[0]]
    assert any(a.tobytes() != b.tobytes() for a, b in zip(before, after)), 'the step did not reach the packed engine'
    for a, b in zip(after, want):
        assert a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------------------------ 7: refusals
def test_refusals(g33, engine, fixture_decoder):
    import torch
    from core.sdfrenderer import SDFRenderer
    from distr import binding, decoder_pack, functions
    from test_gpu_train import _module
    Ws, bs, latent = fixture_decoder
    H, W, K = int(g33['H']), int(g33['W']), g33['K']
    kw = dict(img_hw=(H, W), march_step=int(g33['march_step']), buffer_size=int(g33['buffer_size']))
    dec = _module(Ws, bs)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda().requires_grad_(True)
    lat, R, T = t(latent), t(g33['R']), t(g33['T'])
    # autograd normals: refused unless they are detached; normals from depth are named as supported
    r = SDFRenderer(dec, K, use_depth2normal=False, decoder_grad=True, **kw)
    with pytest.raises(NotImplementedError, match='normals from depth'):
        r.render(lat, R, T)
    depth, normal, mask, q = r.render(lat, R, T, no_grad_normal=True)
    (depth[mask.bool()].sum() + q.sum()).backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in dec.parameters()) and dec.lin0.weight.grad.abs().max() > 0
    r.render_depth(lat, R, T)                                                    # no normals: taken
    # together with normal_decoder_grad
    r.normal_decoder_grad = True
    with pytest.raises(NotImplementedError, match='normal_decoder_grad'):
        r.render_depth(lat, R, T)
    r.normal_decoder_grad = False
    # nothing to do: no decoder parameter requires grad, or grad is off -- taken, and the flag changes nothing
    with torch.no_grad():
        r.render(lat, R, T)
    # another arithmetic
    r2 = SDFRenderer(dec, K, use_depth2normal=True, decoder_grad=True, arith='bf16x6', **kw)
    with pytest.raises(NotImplementedError, match="arith='f32' only"):
        r2.render(lat, R, T)
    # row bands
    weights = [w.requires_grad_(True) for w in _weights(Ws, bs)]
    band = binding.make_cfg((H, W), K, march_step=24, buffer_size=3, want_normal=False, marcher='recursive', band=(8, 16))
    with pytest.raises(NotImplementedError, match='row bands'):
        functions.render_call(engine, band, lat, R, T, weights=weights)
    with pytest.raises(ValueError, match='18 tensors'):
        functions.render_call(engine, binding.make_cfg((H, W), K, march_step=24, buffer_size=3, want_normal=False, marcher='recursive'), lat, R, T, weights=weights[:5])
    # a decoder in training mode with dropout raises as everywhere
    drop = _module(Ws, bs, dropout=list(range(8)), dropout_prob=0.2)
    r3 = SDFRenderer(drop, K, use_depth2normal=True, decoder_grad=True, **kw)
    drop.train()
    with pytest.raises(decoder_pack.UnsupportedDecoder, match='training mode'):
        r3.render(lat, R, T)
