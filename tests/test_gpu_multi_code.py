"""Many shape codes in one launch sequence: decode_sdf_batch / decode_sdf_gradient_batch (distr_mlp_*_multi).

The contract is byte equality with the single-code calls, segment by segment, so every pin the single-code path has (golden G2 / G11,
the code-length embeddings) carries over; one direct comparison with the torch Decoder restates G11's bars. The segment sizes are the
smallest at which a tile -> segment map can go wrong: a lone point, exactly one 64-point tile, one point over, an EMPTY segment in the
middle, three tiles, one short of a tile. Three decoders: the C = 256 fixture, a wide one (C = 64: its own tile layout) and a narrow
non-default one (C = 300).
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = [1, 64, 65, 0, 130, 63]
CODE_LENGTHS = (256, 64, 300)


def _module(Ws, bs):
    import torch
    from core.graph.deep_sdf_decoder import Decoder
    from distr import decoder_pack
    dec = Decoder(decoder_pack.latent_size_of(Ws), [512] * 8, norm_layers=(), latent_in=[4])
    dec.load_state_dict({('lin%d.%s' % (l, n)): torch.from_numpy(a) for l, (W_, b) in enumerate(zip(Ws, bs)) for n, a in (('weight', W_), ('bias', b))})
    return dec.cuda().eval()


@pytest.fixture(scope='module', params=CODE_LENGTHS)
def case(request, fixture_decoder):
    """(decoder module, codes (6, C), points (sum SIZES, 3), upstream gradient (sum SIZES, 1)): made once per code length, never modified."""
    import torch
    from distr import fixture
    Cn = request.param
    Ws, bs, latent = fixture_decoder if Cn == 256 else fixture.make_decoder_weights(latent_size=Cn)
    rs = np.random.RandomState(100 + Cn)
    codes = (latent + 0.3 * np.abs(latent).max() * rs.standard_normal((len(SIZES), Cn))).astype(np.float32)
    pts = ((rs.rand(sum(SIZES), 3) - 0.5) * 1.6).astype(np.float32)
    w = rs.standard_normal((sum(SIZES), 1)).astype(np.float32)
    return _module(Ws, bs), torch.from_numpy(codes).cuda(), torch.from_numpy(pts).cuda(), torch.from_numpy(w).cuda()


def _segments(sizes=SIZES):
    at = 0
    for s, n in enumerate(sizes):
        yield s, at, at + n
        at += n


@pytest.mark.parametrize('clamp', [0.1, None])
def test_forward_equals_single_calls(case, clamp):
    import torch
    from core.utils.decoder_utils import decode_sdf, decode_sdf_batch
    dec, codes, pts, _ = case
    out = decode_sdf_batch(dec, codes, pts, counts=SIZES, clamp_dist=clamp, no_grad=True)
    assert out.shape == (sum(SIZES), 1)
    for s, a, b in _segments():
        assert torch.equal(out[a:b], decode_sdf(dec, codes[s:s + 1], pts[a:b], clamp_dist=clamp, no_grad=True)), s
    assert out.abs().max() > 0 and (clamp is None or out.abs().max() <= clamp)


def test_point_gradient_equals_single_calls(case):
    import torch
    from core.utils.decoder_utils import decode_sdf_gradient, decode_sdf_gradient_batch
    dec, codes, pts, _ = case
    g = decode_sdf_gradient_batch(dec, codes, pts, counts=torch.tensor(SIZES), clamp_dist=0.1)
    assert g.shape == (sum(SIZES), 3) and not g.requires_grad
    for s, a, b in _segments():
        assert torch.equal(g[a:b], decode_sdf_gradient(dec, codes[s:s + 1], pts[a:b], clamp_dist=0.1)), s
    assert g.abs().max() > 0


@pytest.mark.parametrize('clamp', [0.1, None])
def test_backward_equals_single_calls(case, clamp):
    import torch
    from core.utils.decoder_utils import decode_sdf, decode_sdf_batch
    dec, codes, pts, w = case
    lat = codes.clone().requires_grad_(True)
    x = pts.clone().requires_grad_(True)
    (decode_sdf_batch(dec, lat, x, counts=SIZES, clamp_dist=clamp) * w).sum().backward()
    assert lat.grad.shape == codes.shape and x.grad.shape == pts.shape
    for s, a, b in _segments():
        if a == b:
            assert not lat.grad[s].any(), 'the empty segment has a latent gradient'
            continue
        l1 = codes[s:s + 1].clone().requires_grad_(True)
        x1 = pts[a:b].clone().requires_grad_(True)
        (decode_sdf(dec, l1, x1, clamp_dist=clamp) * w[a:b]).sum().backward()
        assert torch.equal(x.grad[a:b], x1.grad), s
        assert torch.equal(lat.grad[s:s + 1], l1.grad), s
    assert x.grad.abs().max() > 0 and lat.grad.abs().max() > 0


def test_shared_code_rows_equal_single_calls(case):
    """latent_stride 0: one code for every segment; g_latent still has one row per segment, each the stand-alone call's."""
    import torch
    from core.utils.decoder_utils import decode_sdf, _engine
    from distr import functions
    dec, codes, pts, w = case
    eng = _engine(dec, pts)
    code = codes[2:3]
    out = functions.mlp_eval_multi(eng, code, pts, SIZES, 0.1)
    g_rows, g_x = functions.mlp_backward_multi(eng, code, pts, SIZES, w, 0.1)
    assert g_rows.shape == (len(SIZES), codes.shape[1])
    for s, a, b in _segments():
        if a == b:
            assert not g_rows[s].any()
            continue
        l1 = code.clone().requires_grad_(True)
        x1 = pts[a:b].clone().requires_grad_(True)
        y1 = decode_sdf(dec, l1, x1, clamp_dist=0.1)
        (y1 * w[a:b]).sum().backward()
        assert torch.equal(out[a:b], y1.detach()) and torch.equal(g_x[a:b], x1.grad) and torch.equal(g_rows[s:s + 1], l1.grad), s
    # the autograd node hands a shared code the sum of the rows
    l2 = code.clone().requires_grad_(True)
    (functions.mlp_eval_multi_autograd(eng, l2, pts, SIZES, 0.1) * w).sum().backward()
    assert torch.equal(l2.grad, g_rows.sum(0).reshape(1, -1))


def test_input_forms_give_the_same_bytes(case):
    import torch
    from core.utils.decoder_utils import decode_sdf_batch, decode_sdf_gradient_batch
    dec, codes, pts, _ = case
    S, N = 4, 65
    x3 = pts[:S * N].reshape(S, N, 3)
    a = decode_sdf_batch(dec, codes[:S], x3, no_grad=True)
    b = decode_sdf_batch(dec, codes[:S], x3.reshape(-1, 3), counts=[N] * S, no_grad=True)
    assert a.shape == (S, N, 1) and b.shape == (S * N, 1) and torch.equal(a.reshape(-1, 1), b)
    ga = decode_sdf_gradient_batch(dec, codes[:S], x3)
    gb = decode_sdf_gradient_batch(dec, codes[:S], x3.reshape(-1, 3), counts=[N] * S)
    assert ga.shape == (S, N, 3) and torch.equal(ga.reshape(-1, 3), gb)


def test_chunks_of_64_segments(case):
    """S = 65 segments of 3 points: two calls (64 + 1) behind one decode_sdf_batch, equal to the per-segment loop."""
    import torch
    from core.utils.decoder_utils import decode_sdf, decode_sdf_batch
    dec, codes, pts, w = case
    S, N = 65, 3
    rs = np.random.RandomState(7)
    lat65 = (codes[torch.from_numpy(rs.randint(0, len(SIZES), S)).cuda()] * torch.from_numpy(rs.uniform(0.5, 1.5, (S, 1)).astype(np.float32)).cuda()).contiguous()
    x65 = pts[:S * N].reshape(S, N, 3)
    lat = lat65.clone().requires_grad_(True)
    x = x65.clone().requires_grad_(True)
    y = decode_sdf_batch(dec, lat, x, clamp_dist=None)
    (y * w[:S * N].reshape(S, N, 1)).sum().backward()
    for s in range(S):
        l1 = lat65[s:s + 1].clone().requires_grad_(True)
        x1 = x65[s].clone().requires_grad_(True)
        y1 = decode_sdf(dec, l1, x1, clamp_dist=None)
        (y1 * w[s * N:(s + 1) * N]).sum().backward()
        assert torch.equal(y[s].detach(), y1.detach()) and torch.equal(x.grad[s], x1.grad) and torch.equal(lat.grad[s:s + 1], l1.grad), s


def test_against_torch_decoder(fixture_decoder):
    """Values and gradients of one batched call against autograd through the torch Decoder, at the bars of golden G11's test
    (tests/test_gpu_parity.py::test_decode_sdf_autograd_matches_reference_golden, restated): sdf to 2e-6; per-point gradients within
    2e-5 of the largest one for all but at most one point (a unit whose pre-activation is ~1e-8 may sit on either side of the ReLU in
    two f32 summation orders); the latent gradient to 2e-3 where such a point was seen, and else to G11's tight bar, max(2 x the
    reference's own noise floor for G11 (tests/golden/noise_floor_g4_g5_g9_g11.npz), 5e-6). The latent bar is applied twice: to
    all rows at once, relative to the largest entry, as G11 does for its single row; and to every non-empty segment's row relative to
    that row's largest entry, with the segment's own flipped points choosing the branch, so that a wrong small row cannot hide behind a
    large one."""
    import os
    import torch
    from conftest import ROOT
    from core.utils.decoder_utils import decode_sdf_batch
    floors = np.load(os.path.join(ROOT, 'tests', 'golden', 'noise_floor_g4_g5_g9_g11.npz'))
    Ws, bs, latent = fixture_decoder
    dec = _module(Ws, bs)
    rs = np.random.RandomState(11)
    sizes = [259, 0, 70, 448]                      # 777 points, as G11
    codes = torch.from_numpy((latent + 0.3 * np.abs(latent).max() * rs.standard_normal((len(sizes), 256))).astype(np.float32)).cuda()
    pts = torch.from_numpy(((rs.rand(sum(sizes), 3) - 0.5) * 1.6).astype(np.float32)).cuda()
    w = torch.from_numpy(rs.standard_normal((sum(sizes), 1)).astype(np.float32)).cuda()
    for name, clamp in (('clamped', 0.1), ('raw', None)):
        tight = max(2.0 * float(floors['g11_g_latent_%s_rel' % name]), 5e-6)
        lat = codes.clone().requires_grad_(True)
        x = pts.clone().requires_grad_(True)
        y = decode_sdf_batch(dec, lat, x, counts=sizes, clamp_dist=clamp)
        (y * w).sum().backward()
        lr = codes.clone().requires_grad_(True)
        xr = pts.clone().requires_grad_(True)
        rows = torch.repeat_interleave(lr, torch.tensor(sizes, device='cuda'), dim=0)
        yr = dec.inference(torch.cat([rows, xr], 1))
        if clamp is not None:
            yr = torch.clamp(yr, -clamp, clamp)
        (yr * w).sum().backward()
        assert (y.detach() - yr.detach()).abs().max().item() <= 2e-6
        ref = xr.grad.cpu().numpy()
        bad = np.abs(x.grad.cpu().numpy() - ref).max(1) > 2e-5 * np.abs(ref).max()
        nbad = int(bad.sum())
        refl = lr.grad.cpu().numpy()
        errl = np.abs(lat.grad.cpu().numpy() - refl)
        rel_l = errl.max() / np.abs(refl).max()
        per_row = [(s, int(bad[a:b].sum()), errl[s].max() / np.abs(refl[s]).max()) for s, a, b in _segments(sizes) if b > a]
        print('%s: points off by > 2e-5: %d of %d; g_latent residual %.3e, per segment (segment, flipped points, residual) %s; tight bar %.3e'
              % (name, nbad, sum(sizes), rel_l, ' '.join('(%d, %d, %.3e)' % r for r in per_row), tight))
        assert nbad <= 1, nbad
        assert rel_l <= (2e-3 if nbad else tight), rel_l
        for s, nbad_s, rel_s in per_row:
            assert rel_s <= (2e-3 if nbad_s else tight), (s, rel_s)
        assert not lat.grad[1].any()


def test_per_view_codes_take_one_decoder_launch(fixture_decoder):
    """get_samples_batch of 3 views of 24 x 24 with a code per view: ONE decoder-evaluation launch in the forward (the launches that
    distr_profile_enable brackets are the decoder / march launches; distr_profile_read counts them). It used to be one per view.
    Only the forward is counted: the profile does not bracket the launches of the point-list backward."""
    import torch
    from core.sdfrenderer import SDFRenderer_deepsdf
    from distr import fixture
    Ws, bs, latent = fixture_decoder
    dec = _module(Ws, bs)
    h = w = 24
    V = 3
    ren = SDFRenderer_deepsdf(dec, fixture.make_intrinsic(h, w), img_hw=(h, w))
    rs = np.random.RandomState(5)
    lat = torch.from_numpy((latent + 0.1 * np.abs(latent).max() * rs.standard_normal((V, 256))).astype(np.float32)).cuda()
    RT = torch.stack([torch.from_numpy(np.concatenate([R, np.asarray(T, np.float32).reshape(3, 1)], 1).astype(np.float32))
                      for R, T in (fixture.make_camera(30 + 20 * v, 20, 1.6, 10) for v in range(V))]).cuda()
    depth = torch.full((V, h, w), 1.2, device='cuda')
    normal = torch.zeros(V, h, w, 3, device='cuda')
    normal[..., 2] = -1.0
    eta = torch.full((V * h * w,), 0.01, device='cuda')
    ctx = ren._engine.ctx
    single = [torch.cat(ren.get_samples(lat[v:v + 1], RT[v], depth[v], normal[v], eta_map=eta[:h * w])) for v in range(V)]
    ctx.profile_enable(True)
    try:
        ctx.profile_read()
        out = ren.get_samples_batch(lat, RT, depth, normal, eta_map=eta)
        n, _ = ctx.profile_read()
    finally:
        ctx.profile_enable(False)
    assert n == 1, 'decoder-evaluation launches of one get_samples_batch forward: %d' % n
    for v in range(V):
        assert torch.equal(torch.cat(out[v]), single[v]), v


def test_multi_c_abi_error_paths(engine):
    """nseg 0 / 65, a negative count, a workspace that is too small: the documented code and a text, nothing launched."""
    import torch
    from distr import binding
    L, h = engine.ctx.L, engine.ctx.h
    p, s = binding.ptr, engine.ctx.stream()
    lat = torch.zeros(2, 256, device='cuda')
    x = torch.zeros(8, 3, device='cuda')
    out = torch.empty(8, device='cuda')
    g = torch.empty(8, 3, device='cuda')
    gl = torch.empty(2, 256, device='cuda')
    ok = (C.c_int64 * 2)(5, 3)
    neg = (C.c_int64 * 2)(9, -1)
    many = (C.c_int64 * 65)(*([0] * 65))
    need_f, need_b = L.distr_mlp_multi_workspace_bytes(2, ok), L.distr_mlp_backward_multi_workspace_bytes(2, ok)
    assert 0 < need_f < need_b
    ws = torch.empty(need_b, dtype=torch.uint8, device='cuda')

    def calls(nseg, cnt, nbytes_f, nbytes_b):
        yield 'eval', L.distr_mlp_eval_multi(h, nseg, cnt, p(lat), 256, p(x), 0.1, p(out), p(ws), nbytes_f, s)
        yield 'grad', L.distr_mlp_grad_multi(h, nseg, cnt, p(lat), 256, p(x), p(out), p(g), p(ws), nbytes_f, s)
        yield 'backward', L.distr_mlp_backward_multi(h, nseg, cnt, p(lat), 256, p(x), p(out), 0.1, p(g), p(gl), p(ws), nbytes_b, s)

    INVALID, WORKSPACE = -1, -4          # DISTR_ERR_INVALID_ARG, DISTR_ERR_WORKSPACE (include/distr.h)
    for nseg, cnt, word in ((0, ok, 'nseg'), (65, many, 'nseg'), (2, neg, 'negative')):
        assert L.distr_mlp_multi_workspace_bytes(nseg, cnt) == 0 and L.distr_mlp_backward_multi_workspace_bytes(nseg, cnt) == 0
        for name, rc in calls(nseg, cnt, need_f, need_b):
            err = L.distr_last_error(h).decode()
            assert rc == INVALID and word in err, (name, nseg, rc, err)
    for name, rc in calls(2, ok, need_f - 1, need_b - 1):
        err = L.distr_last_error(h).decode()
        assert rc == WORKSPACE and 'workspace' in err, (name, rc, err)
    for name, rc in calls(2, ok, need_f, need_b):          # and the same arguments with enough workspace pass
        assert rc == 0, (name, L.distr_last_error(h).decode())
    torch.cuda.synchronize()
