"""SDFRenderer_deepsdf on the GPU (core/sdfrenderer/renderer_deepsdf.py, include/distr_samples.h): golden G31 from the reference, the
composition of the helpers that already ship, byte identity (batch = stand-alone calls, run = run), the random draws, refusals and a
five-step fit.

Bars. Outputs: per sample max(2 x the floor G31 records for the case, 2e-6) (2e-6: the bar of
test_decode_sdf_matches_reference_golden for the same decoder outputs). Gradients: 2 x the recorded floor, relative to the gradient's
largest entry; when ONE sample sits on a ReLU knife edge (its point gradient differs by more than 2e-5 of the largest, the criterion of
test_decode_sdf_autograd_matches_reference_golden) the summed gradients get that test's 2e-3 instead; two such samples fail. The
comparisons with the composed helpers have no floor of their own and use the ones of the matching F1 case of G31.

How tight that is. In every SURFACE case of G31 one of the three noise draws flips a ReLU of one sample (the generator prints the
counts), and that flip is part of the recorded gradient floors: g_latent 3.8e-4 .. 1.7e-3, g_R / g_T 7e-5 .. 1.1e-3, so 2 x floor
reaches 3.3e-3 there -- looser than the 2e-3 knife-edge allowance. The surface gradients are therefore held to about 0.3 % only; the
tight check of the camera pull-back (k_samp_cam_bwd / k_samp_cam_fin share their code between the two modes, the mode only selects
the per-point depth factor) is the FREE-SPACE cases, whose floors are near 1e-6, and the byte-identity test."""
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

H, W = 40, 48


def _g31():
    return dict(np.load(os.path.join(GOLDEN, 'g31_depth_samples.npz')))


def _module(Ws, bs):
    import torch
    from core.graph.deep_sdf_decoder import Decoder
    from distr import decoder_pack
    dec = Decoder(decoder_pack.latent_size_of(Ws), [512] * 8, norm_layers=(), latent_in=[4])
    dec.load_state_dict({('lin%d.%s' % (l, n)): torch.from_numpy(a) for l, (W_, b) in enumerate(zip(Ws, bs)) for n, a in (('weight', W_), ('bias', b))})
    return dec.cuda().eval()


def _renderer(dec, h=H, w=W):
    from core.sdfrenderer import SDFRenderer_deepsdf
    from distr import fixture
    return SDFRenderer_deepsdf(dec, fixture.make_intrinsic(h, w), img_hw=(h, w))


def _t(a, grad=False):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda().requires_grad_(grad)


def _point_grads(ren, lat, points, clamp, w):
    """Per-sample gradient of (w . f(points)).sum() w.r.t. the points the call evaluated (the knife-edge criterion)."""
    import torch
    from distr import functions
    x = points.detach().clone().requires_grad_(True)
    y = functions.mlp_eval_autograd(ren._engine, lat.detach(), x, clamp)
    (y.reshape(-1) * w).sum().backward()
    return x.grad.cpu().numpy()


def _check_grads(tag, got, ref, nbad, floors):
    """got / ref: dicts g_latent, g_R, g_T; floors: the same keys + '_rel' -> the recorded relative floors."""
    assert nbad <= 1, '%s: %d samples on a ReLU knife edge (one is allowed)' % (tag, nbad)
    for k in ('g_latent', 'g_R', 'g_T'):
        rel = float(np.abs(got[k] - ref[k]).max() / np.abs(ref[k]).max())
        bar = 2e-3 if nbad else 2.0 * floors[k + '_rel']
        print('%s %s: residual %.3e (reference noise floor %.3e, bar %.3e, knife-edge samples %d)' % (tag, k, rel, floors[k + '_rel'], bar, nbad))
        assert rel <= bar, (tag, k, rel, bar)


def _run(ren, kind, lat, RT, depth, normal, clamp, draws, w, number=1):
    """One call + backward of (w . out).sum(): out (numpy), gradients, the point list."""
    import torch
    if kind == 'samples':
        pos, neg = ren.get_samples(lat, RT, depth, normal, clamp_dist=clamp, eta_map=draws)
        out = torch.cat([pos, neg])
    else:
        out = ren.get_freespace_samples(lat, RT, depth, clamp_dist=clamp, number=number, ratio=draws)
    (out * w).sum().backward()
    g = dict(g_latent=lat.grad.cpu().numpy().copy(), g_R=RT.grad[:, :3].cpu().numpy().copy(), g_T=RT.grad[:, 3].cpu().numpy().copy())
    return out.detach().cpu().numpy(), g, ren._last_points


@pytest.mark.parametrize('fx', ('f1', 'f2'))
def test_g31_matches_reference_golden(fx, fixture_decoder):
    """G31: values (order and N exact, per-sample bar) and gradients w.r.t. the latent code and RT against the reference."""
    from distr import fixture
    g = _g31()
    Ws, bs, _ = fixture_decoder if fx == 'f1' else fixture.load_fixture_f2()
    assert fixture.weights_sha256(Ws, bs) == str(g[fx + '_weights_sha256'])
    ren = _renderer(_module(Ws, bs))
    N = int(g[fx + '_N'])
    for name in [str(c) for c in g['case_names']]:
        key = '%s_%s_' % (fx, name)
        kind = 'samples' if name.startswith('s_') else 'free'
        clamp = float(g[key + 'clamp_dist'])
        lat, RT = _t(g[fx + '_latent'], True), _t(g[fx + '_RT'], True)
        draws = _t(g[key + 'eta_map'] if kind == 'samples' else g[key + 'ratio'])
        w = _t(g[key + 'w'])
        number = 1 if kind == 'samples' else g[key + 'ratio'].shape[0]
        out, grads, pts = _run(ren, kind, lat, RT, _t(g[fx + '_depth']), _t(g[fx + '_normal']), clamp, draws, w, number)
        assert ren.last_counts == [N] and out.shape == g[key + 'out'].shape
        err = np.abs(out - g[key + 'out'])
        bar = max(2.0 * float(g[key + 'floor_out']), 2e-6)
        print('G31 %s values: max residual %.3e (reference noise floor %.3e, bar %.3e)' % (key, err.max(), float(g[key + 'floor_out']), bar))
        assert err.max() <= bar, (key, err.max(), bar)
        ref_gp = g[key + 'g_points']
        gp = _point_grads(ren, lat, pts, clamp, w)
        nbad = int((np.abs(gp - ref_gp).max(1) > 2e-5 * np.abs(ref_gp).max()).sum())
        ref = dict(g_latent=g[key + 'g_latent'], g_R=g[key + 'g_RT'][:, :3], g_T=g[key + 'g_RT'][:, 3])
        _check_grads('G31 ' + key, grads, ref, nbad, {k + '_rel': float(g[key + 'floor_' + k + '_rel']) for k in ref})


def _composed(ren, dec, kind, lat, RT, depth, normal, clamp, draws, number):
    """The same quantities from the helpers that already ship, under autograd. Returns (out, points)."""
    import torch
    from core.utils.decoder_utils import decode_sdf
    R, T = RT[:, :3], RT[:, 3]
    cam_pos, rays = ren.get_camera_location(R, T), ren.get_camera_rays(R)
    d = depth.reshape(-1)
    valid = (d > 0) & (d < 1e5)
    z = d[valid] / ren.calib_map[valid]
    if kind == 'samples':
        p = ren.generate_point_samples(cam_pos, rays[:, valid], z, has_zdepth_grad=False).t()
        off = ren.inv_transform_points(normal.reshape(-1, 3)[valid].t()).t() * draws[:, None]
        pts = torch.cat([p + off, p - off])
        sign = torch.cat([-draws, draws])
    else:
        pts = torch.cat([ren.generate_point_samples(cam_pos, rays[:, valid], z * draws.reshape(number, -1)[k], has_zdepth_grad=False).t() for k in range(number)])
        sign = torch.zeros(pts.shape[0], device=pts.device)
    pts.retain_grad()
    return decode_sdf(dec, lat, pts, clamp_dist=clamp).squeeze(-1) + sign, pts


@pytest.mark.parametrize('C', (64, 256, 300))
def test_equals_composed_helpers(C):
    """get_samples / get_freespace_samples against get_camera_location, get_camera_rays, generate_point_samples, inv_transform_points
    and decode_sdf under autograd: random cameras, code lengths on both decoder layouts; points at a few ulp, outputs and gradients at
    the bars of the matching G31 case."""
    import torch
    from distr import fixture
    g = _g31()
    Ws, bs, latent = fixture.make_decoder_weights(latent_size=C)
    dec = _module(Ws, bs)
    ren = _renderer(dec)
    rs = np.random.RandomState(100 + C)
    for trial in range(2):
        R, T = fixture.make_camera(rs.uniform(-60, 60), rs.uniform(-40, 40), rs.uniform(1.4, 1.9), rs.uniform(-30, 30))
        RT0 = np.concatenate([R, T.reshape(3, 1)], 1)
        lat_obs = latent + 0.02 * np.abs(latent).max() * rs.standard_normal(latent.shape)
        with torch.no_grad():
            depth, normal = ren.render(_t(lat_obs), _t(R), _t(T))[:2]
        depth, normal = depth.detach(), normal.detach()
        N = int(((depth > 0) & (depth < 1e5)).sum())
        assert N > 50
        for kind, number, clamp, case in (('samples', 1, 0.1, 's_rand'), ('samples', 1, 0.004, 's_clamp'), ('free', 3, 0.5, 'f_n3')):
            m = 2 if kind == 'samples' else number
            draws = _t(rs.random_sample(m * N // (2 if kind == 'samples' else 1)) * (0.01 if kind == 'samples' else 1.0))
            w = _t(rs.uniform(0.5, 1.5, m * N) * rs.choice([-1.0, 1.0], m * N))
            lat, RT = _t(latent, True), _t(RT0, True)
            out, grads, pts = _run(ren, kind, lat, RT, depth, normal, clamp, draws, w, number)
            lat2, RT2 = _t(latent, True), _t(RT0, True)
            out2, pts2 = _composed(ren, dec, kind, lat2, RT2, depth, normal, clamp, draws, number)
            (out2 * w).sum().backward()
            assert out.shape == tuple(out2.shape)
            perr = float((pts - pts2.detach()).abs().max())
            print('C %d trial %d %s: points differ by at most %.3e' % (C, trial, kind, perr))
            assert perr <= 4 * 2.0 ** -23 * max(1.0, float(pts2.detach().abs().max()))          # a few ulp of the largest coordinate
            key = 'f1_%s_' % case
            bar = max(2.0 * float(g[key + 'floor_out']), 2e-6)
            err = float(np.abs(out - out2.detach().cpu().numpy()).max())
            print('C %d trial %d %s values: max residual %.3e (bar %.3e)' % (C, trial, case, err, bar))
            assert err <= bar
            ref_gp = pts2.grad.cpu().numpy()
            gp = _point_grads(ren, lat, pts, clamp, w)
            nbad = int((np.abs(gp - ref_gp).max(1) > 2e-5 * np.abs(ref_gp).max()).sum())
            ref = dict(g_latent=lat2.grad.cpu().numpy(), g_R=RT2.grad[:, :3].cpu().numpy(), g_T=RT2.grad[:, 3].cpu().numpy())
            _check_grads('C %d trial %d %s' % (C, trial, case), grads, ref, nbad, {k + '_rel': float(g[key + 'floor_' + k + '_rel']) for k in ref})


def _scene(ren, latent, views, seed):
    """V observed views of a nearby code: (RT (V,3,4), depth (V,H,W), normal (V,H,W,3))."""
    import torch
    from distr import fixture
    rs = np.random.RandomState(seed)
    lat_obs = _t(latent + 0.02 * np.abs(latent).max() * rs.standard_normal(latent.shape))
    RTs, ds, ns = [], [], []
    for v in range(views):
        R, T = fixture.make_camera(-50 + 45 * v, 10 + 12 * v, 1.5 + 0.1 * v, 8 * v)
        with torch.no_grad():
            d, n = ren.render(lat_obs, _t(R), _t(T))[:2]
        RTs.append(np.concatenate([R, T.reshape(3, 1)], 1)); ds.append(d.detach()); ns.append(n.detach())
    return _t(np.stack(RTs)), torch.stack(ds), torch.stack(ns)


@pytest.mark.parametrize('per_view_codes', (False, True))
def test_batch_equals_stand_alone_calls_and_runs_repeat(per_view_codes, fixture_decoder):
    """Every view's slice of a batch is byte for byte its stand-alone call, forward and backward; two runs give the same bytes."""
    import torch
    Ws, bs, latent = fixture_decoder
    ren = _renderer(_module(Ws, bs))
    V = 3
    RT, depth, normal = _scene(ren, latent, V, 7)
    rs = np.random.RandomState(8)
    codes = np.concatenate([latent + 0.01 * np.abs(latent).max() * rs.standard_normal(latent.shape) for _ in range(V)]) if per_view_codes else latent
    counts = [int(((depth[v] > 0) & (depth[v] < 1e5)).sum()) for v in range(V)]
    for kind, number in (('samples', 1), ('free', 3)):
        m = 2 if kind == 'samples' else number
        draws = [_t(rs.random_sample((m if kind == 'free' else 1) * c) * (0.01 if kind == 'samples' else 1.0)) for c in counts]
        ws = [_t(rs.uniform(-1.5, 1.5, m * c)) for c in counts]

        def batch():
            lat, rt = _t(codes, True), RT.detach().clone().requires_grad_(True)
            if kind == 'samples':
                outs = [torch.cat(o) for o in ren.get_samples_batch(lat, rt, depth, normal, clamp_dist=0.05, eta_map=draws)]
            else:
                outs = ren.get_freespace_samples_batch(lat, rt, depth, clamp_dist=0.3, number=number, ratio=draws)
            sum((o * w).sum() for o, w in zip(outs, ws)).backward()
            return [o.detach().cpu().numpy() for o in outs], lat.grad.cpu().numpy(), rt.grad.cpu().numpy()
        outs, g_lat, g_rt = batch()
        outs2, g_lat2, g_rt2 = batch()
        assert ren.last_counts == counts
        assert all(a.tobytes() == b.tobytes() for a, b in zip(outs, outs2)) and g_lat.tobytes() == g_lat2.tobytes() and g_rt.tobytes() == g_rt2.tobytes()
        for v in range(V):
            lat = _t(codes[v:v + 1] if per_view_codes else codes, True)
            rt = RT[v].detach().clone().requires_grad_(True)
            if kind == 'samples':
                o = torch.cat(ren.get_samples(lat, rt, depth[v], normal[v], clamp_dist=0.05, eta_map=draws[v]))
            else:
                o = ren.get_freespace_samples(lat, rt, depth[v], clamp_dist=0.3, number=number, ratio=draws[v])
            (o * ws[v]).sum().backward()
            assert o.detach().cpu().numpy().tobytes() == outs[v].tobytes(), (kind, v)
            assert rt.grad.cpu().numpy().tobytes() == g_rt[v].tobytes(), (kind, v)
            if per_view_codes:          # (a shared code's gradient is the sum over the views: nothing per view to compare)
                assert lat.grad.cpu().numpy().tobytes() == g_lat[v:v + 1].tobytes(), (kind, v)


def test_compaction_order_and_c_abi_refusals(engine, fixture_decoder):
    """distr_depth_samples_count: row-major order and counts against torch.nonzero, through the session engine; bad arguments get the
    library's error codes and text."""
    import ctypes as C
    import torch
    from distr import binding, fixture, functions
    rs = np.random.RandomState(3)
    h, w = 37, 61                                      # more than one block of 2048 pixels, ragged
    d = rs.uniform(0.5, 2.0, (2, h, w)).astype(np.float32)
    d[rs.random_sample(d.shape) < 0.4] = 1e11
    d[rs.random_sample(d.shape) < 0.1] = 0.0
    d[0, 0, 0], d[1, -1, -1] = np.nan, -1.0
    cfg = binding.make_samples_cfg((h, w), fixture.make_intrinsic(h, w), np.eye(3), 0.1, 'surface')
    dt, index, counts = functions.depth_samples_count(engine, cfg, torch.from_numpy(d).cuda())
    for v in range(2):
        want = np.nonzero((d[v].reshape(-1) > 0) & (d[v].reshape(-1) < 1e5))[0]
        assert counts[v] == want.size and np.array_equal(index[v, :counts[v]].cpu().numpy(), want)
    L = engine.ctx.L
    short = binding.make_samples_cfg((h, w), fixture.make_intrinsic(h, w), np.eye(3), 0.1, 'surface')
    short.struct_size -= 4
    nb = C.c_size_t()
    assert L.distr_depth_samples_workspace_bytes(engine.ctx.h, C.byref(short), 1, None, C.byref(nb), None, None) == -1
    assert b'struct_size' in L.distr_last_error(engine.ctx.h)
    assert L.distr_depth_samples_workspace_bytes(engine.ctx.h, C.byref(cfg), 65, None, C.byref(nb), None, None) == -1
    bad = binding.make_samples_cfg((h, w), fixture.make_intrinsic(h, w), np.eye(3), 0.1, 'freespace', number=0)
    assert L.distr_depth_samples_workspace_bytes(engine.ctx.h, C.byref(bad), 1, None, C.byref(nb), None, None) == -1
    assert b'number' in L.distr_last_error(engine.ctx.h)


def test_random_draws_follow_the_torch_seed(fixture_decoder):
    import torch
    Ws, bs, latent = fixture_decoder
    ren = _renderer(_module(Ws, bs))
    RT, depth, normal = _scene(ren, latent, 1, 11)
    lat = _t(latent)
    with torch.no_grad():
        torch.manual_seed(5)
        a = ren.get_samples(lat, RT[0], depth[0], normal[0], eta=0.02)
        eta_a = ren.last_eta_map.clone()
        fa = ren.get_freespace_samples(lat, RT[0], depth[0], number=2)
        torch.manual_seed(5)
        b = ren.get_samples(lat, RT[0], depth[0], normal[0], eta=0.02)
        fb = ren.get_freespace_samples(lat, RT[0], depth[0], number=2)
        torch.manual_seed(6)
        c = ren.get_samples(lat, RT[0], depth[0], normal[0], eta=0.02)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(fa, fb) and not torch.equal(a[0], c[0])
        assert float(eta_a.min()) >= 0.0 and float(eta_a.max()) < 0.02 and eta_a.numel() == ren.last_counts[0]
        assert float(ren.last_ratio.min()) >= 0.0 and float(ren.last_ratio.max()) < 1.0 and fa.numel() == 2 * ren.last_counts[0]
        fixed = ren.get_samples(lat, RT[0], depth[0], normal[0], eta=0.02, use_rand=False)
        given = ren.get_samples(lat, RT[0], depth[0], normal[0], eta_map=torch.full((ren.last_counts[0],), 0.02, device='cuda'))
        assert torch.equal(fixed[0], given[0]) and torch.equal(fixed[1], given[1])


def test_refusals(fixture_decoder):
    import torch
    Ws, bs, latent = fixture_decoder
    ren = _renderer(_module(Ws, bs))
    RT, depth, normal = _scene(ren, latent, 1, 12)
    lat, rt, d, n = _t(latent), RT[0], depth[0], normal[0]
    with pytest.raises(ValueError, match='No valid depth.'):
        ren.get_samples(lat, rt, torch.full_like(d, 1e11), n)
    with pytest.raises(ValueError, match='No valid depth.'):
        ren.get_freespace_samples(lat, rt, torch.zeros_like(d))
    with pytest.raises(ValueError, match='depth requires grad'):
        ren.get_samples(lat, rt, d.clone().requires_grad_(True), n)
    with pytest.raises(ValueError, match='normal requires grad'):
        ren.get_samples(lat, rt, d, n.clone().requires_grad_(True))
    with pytest.raises(ValueError, match='depth requires grad'):
        ren.get_freespace_samples(lat, rt, d.clone().requires_grad_(True))
    with pytest.raises(ValueError, match=r'\(1, 256\)'):
        ren.get_samples(lat[:, :100], rt, d, n)
    with pytest.raises(ValueError, match='img_hw'):
        ren.get_samples(lat, rt, d[:-1], n)
    with pytest.raises(ValueError, match='img_hw'):
        ren.get_freespace_samples(lat, rt, d[:, :-2])


def test_five_adam_steps_reduce_the_residual(fixture_decoder):
    """A perturbed code fitted to a rendered depth / normal map with these residuals alone: mean |clamped residual| after step 5 is
    below step 0."""
    import torch
    Ws, bs, latent = fixture_decoder
    ren = _renderer(_module(Ws, bs), 64, 64)
    from distr import fixture
    R, T = fixture.make_camera(30, 20, 1.6, 10)
    RT = _t(np.concatenate([R, T.reshape(3, 1)], 1))
    with torch.no_grad():
        depth, normal = ren.render(_t(latent), _t(R), _t(T))[:2]
    depth, normal = depth.detach(), normal.detach()
    rs = np.random.RandomState(13)
    lat = _t(latent + np.abs(latent).max() * 0.3 * rs.standard_normal(latent.shape), True)
    opt = torch.optim.Adam([lat], lr=2e-4)
    clamp = 0.1

    def loss_of():
        pos, neg = ren.get_samples(lat, RT, depth, normal, clamp_dist=clamp, eta=0.01, use_rand=False)
        return torch.clamp(torch.cat([pos, neg]), -clamp, clamp).abs().mean()
    losses = []
    for step in range(6):
        loss = loss_of()
        losses.append(float(loss))
        if step < 5:
            opt.zero_grad()
            loss.backward()
            opt.step()
    print('fit: mean |clamped residual| per step', ['%.5e' % l for l in losses])
    assert losses[5] < losses[0], losses
