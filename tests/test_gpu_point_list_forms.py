"""The plain and the segmented point list share one host body (csrc/distr_api.hip: PointList), and render_call is the batched autograd
node with B = 1. These tests hold the two forms of each against one another, byte for byte, at the sizes where the shared body
branches: the empty list, one point, around one 64-point tile, and around the 16-ray route's boundary (tail16_threshold = 4096,
plain list only). tests/test_gpu_multi_code.py compares every segment of a SIX-segment call with the plain call (sizes 1, 64, 65, 130,
63); here the segmented call has ONE segment, and the sizes 0, 4096 and 4097 are added."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 63, 64, 65, 4096, 4097]


@pytest.fixture(scope='module', params=(256, 64))
def case(request, fixture_decoder):
    """(engine, code (1, C), points (4097, 3), upstream gradient (4097, 1)) for the fixture decoder and a wide one (C = 64)."""
    import torch
    from distr import fixture, functions
    Cn = request.param
    Ws, bs, latent = fixture_decoder if Cn == 256 else fixture.make_decoder_weights(latent_size=Cn)
    rs = np.random.RandomState(Cn)
    pts = ((rs.rand(max(SIZES), 3) - 0.5) * 1.6).astype(np.float32)
    w = rs.standard_normal((max(SIZES), 1)).astype(np.float32)
    return (functions.engine_from_weights(Ws, bs, 0), torch.from_numpy(np.asarray(latent, np.float32).reshape(1, Cn)).cuda(),
            torch.from_numpy(pts).cuda(), torch.from_numpy(w).cuda())


@pytest.mark.parametrize('n', SIZES)
def test_plain_list_equals_one_segment(case, n):
    import torch
    from distr import functions
    eng, code, pts, w = case
    x = pts[:n]
    for clamp in (0.1, None):
        assert torch.equal(functions.mlp_eval(eng, code, x, clamp), functions.mlp_eval_multi(eng, code, x, [n], clamp)), clamp
    for a, b in zip(functions.mlp_grad(eng, code, x), functions.mlp_grad_multi(eng, code, x, [n])):
        assert torch.equal(a, b)
    for clamp in (0.1, None):
        grads = []
        for call in (lambda l, p: functions.mlp_eval_autograd(eng, l, p, clamp), lambda l, p: functions.mlp_eval_multi_autograd(eng, l, p, [n], clamp)):
            l1, x1 = code.clone().requires_grad_(True), x.clone().requires_grad_(True)
            (call(l1, x1) * w[:n]).sum().backward()
            grads.append((l1.grad, x1.grad))
        assert torch.equal(grads[0][0], grads[1][0]) and torch.equal(grads[0][1], grads[1][1]), clamp
        assert grads[0][0].shape == code.shape and grads[0][1].shape == (n, 3)
        if n == 0:
            assert not grads[0][0].any() and not grads[1][0].any()
        elif clamp is None:              # (a clamped point has no gradient: only the unclamped run must see some)
            assert grads[0][0].abs().max() > 0 and grads[0][1].abs().max() > 0


def test_unaligned_workspace_of_exactly_the_public_size(engine, fixture_decoder):
    """distr_mlp_backward and distr_color_backward at n = 65 on a workspace of exactly the public size whose base is odd: the carve
    aligns the base up inside the slack the size includes, so the results are those of an aligned workspace."""
    import torch
    from distr import binding, fixture, functions
    n = 65
    rs = np.random.RandomState(3)
    x = torch.from_numpy(((rs.rand(n, 3) - 0.5) * 1.6).astype(np.float32)).cuda()
    Wc, bc, ccode = fixture.make_color_decoder_weights(color_size=8)
    ceng = functions.ColorEngine(weights=(Wc, bc))
    lat = torch.from_numpy(np.asarray(fixture_decoder[2], np.float32).reshape(-1)).cuda()
    clat = torch.cat([lat, torch.from_numpy(np.asarray(ccode, np.float32).reshape(-1)).cuda()])
    g1 = torch.from_numpy(rs.standard_normal(n).astype(np.float32)).cuda()
    g3 = torch.from_numpy(rs.standard_normal((n, 3)).astype(np.float32)).cuda()
    p = binding.ptr
    need = engine.ctx.L.distr_mlp_backward_workspace_bytes(n)

    def run(eng, odd, call):
        buf = torch.empty(need + 1, dtype=torch.uint8, device='cuda')
        ws = buf[1:] if odd else buf[:need]
        assert ws.numel() == need and ws.data_ptr() % 2 == (1 if odd else 0)
        g_x = torch.empty(n, 3, device='cuda')
        g_l = torch.empty(eng.latent_size, device='cuda')
        eng.ctx.check(call(eng, g_x, g_l, ws))
        torch.cuda.synchronize()
        return g_x, g_l

    def sdf(eng, g_x, g_l, ws):
        return eng.ctx.L.distr_mlp_backward(eng.ctx.h, p(lat), p(x), n, p(g1), 0.1, p(g_x), p(g_l), p(ws), ws.numel(), eng.ctx.stream())

    def color(eng, g_x, g_l, ws):
        return eng.ctx.L.distr_color_backward(eng.ctx.h, p(clat), p(x), n, p(g3), p(g_x), p(g_l), p(ws), ws.numel(), eng.ctx.stream())

    for eng, call in ((engine, sdf), (ceng, color)):
        a, b = run(eng, False, call), run(eng, True, call)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), call.__name__
        assert a[0].abs().max() > 0 and a[1].abs().max() > 0


def _module(Ws, bs):
    import torch
    from core.graph.deep_sdf_decoder import Decoder
    dec = Decoder(256, [512] * 8, norm_layers=(), latent_in=[4])
    dec.load_state_dict({('lin%d.%s' % (l, n)): torch.from_numpy(a) for l, (W_, b) in enumerate(zip(Ws, bs)) for n, a in (('weight', W_), ('bias', b))})
    return dec.cuda().eval()


RENDERS = [dict(H=40, W=40, kw=dict(march_step=12, buffer_size=3, marcher='trivial')),
           dict(H=64, W=72, kw=dict(march_step=30, buffer_size=3, marcher='pyramid_recursive'))]


def _render_both(engine, cfg, latent, R, T, Rin, Tin):
    """((outputs, gradients) of render_call, the same of render_batch_call with B = 1); R / T are handed over as Rin(R) / Tin(T)."""
    import torch
    from distr import functions
    res = []
    for single in (True, False):
        l1 = torch.from_numpy(latent).cuda().requires_grad_(True)
        R1, T1 = Rin(R).requires_grad_(True), Tin(T).requires_grad_(True)
        if single:
            out = functions.render_call(engine, cfg, l1, R1, T1)
        else:
            out = functions.render_batch_call(engine, cfg, l1, R1.reshape(1, 3, 3), T1.reshape(1, 3))
        z, mask, q, depth, normal = out
        loss = (z * mask.reshape(z.shape).float()).sum() + q.clamp(max=0.1).sum()
        if cfg.want_normal:
            loss = loss + (depth * 0.5).sum() + (normal * 0.25).sum()
        loss.backward()
        res.append((out, (l1.grad, R1.grad, T1.grad)))
    return res


@pytest.mark.parametrize('want_normal', [True, False])
@pytest.mark.parametrize('case', RENDERS, ids=lambda c: c['kw']['marcher'])
def test_render_call_is_the_batch_node_with_one_view(engine, fixture_decoder, case, want_normal):
    import torch
    from distr import binding, fixture
    H, W = case['H'], case['W']
    P = H * W
    cfg = binding.make_cfg((H, W), fixture.make_intrinsic(H, W), use_depth2normal=True, want_normal=want_normal, **case['kw'])
    R, T = fixture.make_camera(30, 20, 1.6, 10)
    to_dev = lambda a: torch.from_numpy(np.asarray(a, np.float32)).cuda()
    (one, g_one), (bat, g_bat) = _render_both(engine, cfg, fixture_decoder[2], R, T, to_dev, to_dev)
    shapes = [(P,), (P,), (P,), (H, W) if want_normal else (0,), (H, W, 3) if want_normal else (0,)]
    for a, b, sh in zip(one, bat, shapes):
        assert a.shape == sh and torch.equal(a, b.reshape(sh))
    assert one[1].dtype == torch.uint8 and one[1].any()
    for a, b, sh in zip(g_one, g_bat, [(1, 256), (3, 3), (3,)]):
        assert a.shape == sh and a.is_cuda and a.dtype == torch.float32 and torch.equal(a, b.reshape(sh)) and a.abs().max() > 0


def test_render_call_returns_camera_gradients_as_the_inputs_are(engine, fixture_decoder):
    """R and T as float64 host tensors: their gradients come back as float64 host tensors of shapes (3,3) and (3,)."""
    import torch
    from distr import binding, fixture
    cfg = binding.make_cfg((40, 40), fixture.make_intrinsic(40, 40), use_depth2normal=True, **RENDERS[0]['kw'])
    R, T = fixture.make_camera(30, 20, 1.6, 10)
    to_host = lambda a: torch.from_numpy(np.asarray(a, np.float64).copy())
    to_dev = lambda a: torch.from_numpy(np.asarray(a, np.float32)).cuda()
    (_, (gl, gR, gT)), _ = _render_both(engine, cfg, fixture_decoder[2], R, T, to_host, to_host)
    (_, (dl, dR, dT)), _ = _render_both(engine, cfg, fixture_decoder[2], R, T, to_dev, to_dev)
    for g, sh, d in ((gR, (3, 3), dR), (gT, (3,), dT)):
        assert g.shape == sh and g.dtype == torch.float64 and not g.is_cuda and torch.equal(g, d.cpu().double())
    assert torch.equal(gl, dl)
    with pytest.raises(ValueError, match=r'\(3,3\)'):
        from distr import functions
        functions.render_call(engine, cfg, to_dev(fixture_decoder[2]), to_dev(np.stack([R, R])), to_dev(T))


def test_backward_refuses_refreshed_weights_and_engines_count_uploads(engine, fixture_decoder):
    import torch
    from distr import binding, fixture, functions
    Ws, bs, latent = fixture_decoder
    dec = _module(Ws, bs)
    eng = functions.get_engine(dec, 0)
    assert eng.generation >= 1 and eng.latent_size == 256 and engine.generation >= 1 and engine.latent_size == 256
    cfg = binding.make_cfg((40, 40), fixture.make_intrinsic(40, 40), **RENDERS[0]['kw'])
    R, T = (torch.from_numpy(np.asarray(a, np.float32)).cuda() for a in fixture.make_camera(30, 20, 1.6, 10))
    lat = torch.from_numpy(latent).cuda().requires_grad_(True)
    z = functions.render_call(eng, cfg, lat, R, T)[0]
    eng.refresh(dec)
    with pytest.raises(RuntimeError, match='re-uploaded'):
        z.sum().backward()


def _launches(ctx, call):
    ctx.profile_enable(True)
    try:
        ctx.profile_read()
        call()
        return ctx.profile_read()[0]
    finally:
        ctx.profile_enable(False)


def test_bracketed_launch_counts(engine, fixture_decoder):
    """What distr_profile_read counts (the launches MarchTimer brackets), read off the host code before the two list forms shared a
    body: a decoder evaluation is ONE bracketed launch, plain (16-ray route at n = 65, 64-ray tiles at n = 4097) or segmented, and
    so is the forward of the depth samples with a shared code (the per-view form: tests/test_gpu_multi_code.py); the point-list
    backward brackets nothing."""
    import torch
    from core.sdfrenderer import SDFRenderer_deepsdf
    from distr import fixture, functions
    Ws, bs, latent = fixture_decoder
    code = torch.from_numpy(np.asarray(latent, np.float32).reshape(1, 256)).cuda()
    rs = np.random.RandomState(1)
    pts = torch.from_numpy(((rs.rand(4097, 3) - 0.5) * 1.6).astype(np.float32)).cuda()
    g = torch.ones(4097, device='cuda')
    ctx = engine.ctx
    assert _launches(ctx, lambda: functions.mlp_eval(engine, code, pts[:65], 0.1)) == 1
    assert _launches(ctx, lambda: functions.mlp_eval(engine, code, pts, 0.1)) == 1
    assert _launches(ctx, lambda: functions.mlp_eval_multi(engine, code, pts[:130], [65, 0, 65], 0.1)) == 1
    assert _launches(ctx, lambda: functions.mlp_backward_multi(engine, code, pts[:65], [65], g[:65], 0.1)) == 0
    x = pts[:65].clone().requires_grad_(True)
    y = functions.mlp_eval_autograd(engine, code.clone().requires_grad_(True), x, 0.1)
    assert _launches(ctx, lambda: y.sum().backward()) == 0
    h = w = 24
    V = 3
    ren = SDFRenderer_deepsdf(_module(Ws, bs), fixture.make_intrinsic(h, w), img_hw=(h, w))
    RT = torch.stack([torch.from_numpy(np.concatenate([R, np.asarray(T, np.float32).reshape(3, 1)], 1).astype(np.float32))
                      for R, T in (fixture.make_camera(30 + 20 * v, 20, 1.6, 10) for v in range(V))]).cuda()
    depth = torch.full((V, h, w), 1.2, device='cuda')
    normal = torch.zeros(V, h, w, 3, device='cuda')
    normal[..., 2] = -1.0
    eta = torch.full((V * h * w,), 0.01, device='cuda')
    assert _launches(ren._engine.ctx, lambda: ren.get_samples_batch(code, RT, depth, normal, eta_map=eta)) == 1
