"""DeepSDF decoders whose code length C is not 256.

lin3 of a latent_in=[4] decoder has 509 - C rows. C > 256 (narrow layout): packed zero-padded to the 253 rows of the C = 256 tile, the
same kernels. C < 256 (wide layout): padded to 509 rows, lin3 / lin4 run as 512 x 512 layers in their own kernels. Two kinds of checks:
  * embedding: a decoder D_C built to compute exactly what a C = 256 decoder D_256 computes must give BIT-IDENTICAL renders, gradients
    and point values. C > 256: D_256's lin3 rows >= 509 - C are zero, D_C's extra latent columns meet a zero tail of the code. C < 256:
    D_C's lin3 rows 253..508 - C (and their lin4 columns) are zero, D_256's latent columns >= C are zero and its code is [z | 0];
  * dense: the fixture decoder of code length C (every lin3 row non-zero) against the PyTorch restatement at the usual bars.
"""
import json
import os

import numpy as np
import pytest

import helpers

pytestmark = pytest.mark.gpu

CODE_LENGTHS = (64, 128, 255, 300, 508)


def _embedding(fixture_decoder, C):
    """(D_256 weights, D_C weights, z_256, z_C): the same function, once with code length 256 and once with C."""
    if C < 256:
        return _embedding_wide(fixture_decoder, C)
    Ws, bs, z = fixture_decoder
    r3 = 509 - C
    W256 = [W.copy() for W in Ws]
    b256 = [b.copy() for b in bs]
    W256[3][r3:] = 0.0
    b256[3][r3:] = 0.0
    W256[4][:, r3:253] = 0.0
    # lin4's xyz columns (zero in the fixture): with C = 508 lin3 keeps one row, and the field needs them to keep a surface
    W256[4][:, 509:] = np.random.RandomState(C).standard_normal((512, 3)).astype(np.float32) * np.float32(np.sqrt(2.0 / 512))
    WC = [W.copy() for W in W256]
    bC = [b.copy() for b in b256]
    extra = np.zeros((512, C - 256), np.float32)            # the extra latent columns (zero: Adam keeps the code's tail at 0)
    WC[0] = np.ascontiguousarray(np.concatenate([W256[0][:, :256], extra, W256[0][:, 256:]], 1))
    WC[3] = np.ascontiguousarray(W256[3][:r3])
    bC[3] = np.ascontiguousarray(b256[3][:r3])
    WC[4] = np.ascontiguousarray(np.concatenate([W256[4][:, :r3], W256[4][:, 253:509], extra, W256[4][:, 509:]], 1))
    zC = np.concatenate([z, np.zeros((1, C - 256), np.float32)], 1)
    return (W256, b256), (WC, bC), z, zC


def _embedding_wide(fixture_decoder, C):
    Ws, bs, z = fixture_decoder
    r3 = 509 - C                                            # > 253: rows 253.. of D_C's lin3 are zero
    W256 = [W.copy() for W in Ws]
    b256 = [b.copy() for b in bs]
    W256[0][:, C:256] = 0.0                                 # D_256's latent columns behind D_C's: zero (Adam keeps the code's tail at 0)
    W256[4][:, 253 + C:509] = 0.0
    WC = [W.copy() for W in W256]
    bC = [b.copy() for b in b256]
    WC[0] = np.ascontiguousarray(np.concatenate([W256[0][:, :C], W256[0][:, 256:]], 1))
    WC[3] = np.ascontiguousarray(np.concatenate([W256[3], np.zeros((r3 - 253, 512), np.float32)], 0))
    bC[3] = np.ascontiguousarray(np.concatenate([b256[3], np.zeros(r3 - 253, np.float32)]))
    WC[4] = np.ascontiguousarray(np.concatenate([W256[4][:, :253], np.zeros((512, r3 - 253), np.float32), W256[4][:, 253:253 + C],
                                                 W256[4][:, 509:]], 1))
    z256 = np.concatenate([z[:, :C], np.zeros((1, 256 - C), np.float32)], 1)
    return (W256, b256), (WC, bC), z256, np.ascontiguousarray(z[:, :C])


@pytest.fixture(scope='module', params=CODE_LENGTHS)
def pair(request, fixture_decoder):
    from distr import functions
    C = request.param
    (W256, b256), (WC, bC), z, zC = _embedding(fixture_decoder, C)
    e256 = functions.engine_from_weights(W256, b256, 0)
    eC = functions.engine_from_weights(WC, bC, 0)
    assert eC.latent_size == C and e256.latent_size == 256
    return C, e256, eC, z, zC


def _same(a, b, keys):
    for k in keys:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k


@pytest.mark.parametrize('marcher,d2n', [('pyramid_recursive', True), ('pyramid_recursive', False), ('recursive', True), ('recursive', False)])
def test_embedding_render_exact(pair, marcher, d2n):
    from distr import fixture
    C, e256, eC, z, zC = pair
    H = W = 64
    K = fixture.make_intrinsic(H, W)
    R, T = fixture.make_camera(35, 20, 1.6, 10)
    kw = dict(march_step=30, buffer_size=3, marcher=marcher, use_depth2normal=d2n)
    a = helpers.hip_render(e256, H, W, K, R, T, z, **kw)
    b = helpers.hip_render(eC, H, W, K, R, T, zC, **kw)
    assert a['mask'].sum() > 50
    _same(a, b, ('zdepth', 'mask', 'min_sdf', 'depth', 'normal', 'g_R', 'g_T'))
    m = min(C, 256)
    assert b['g_latent'].shape == (1, C)
    assert np.array_equal(a['g_latent'][:, :m], b['g_latent'][:, :m]), 'k_bwd_final: g_latent = W0lat^T sd0 + W4lat^T sd4 differs'
    assert not np.any(b['g_latent'][:, m:]) and not np.any(a['g_latent'][:, m:])


def test_embedding_points_exact(pair):
    import torch
    from distr import functions
    C, e256, eC, z, zC = pair
    rs = np.random.RandomState(3)
    pts = torch.from_numpy((rs.rand(5000, 3).astype(np.float32) - 0.5) * 1.6).cuda()
    out = []
    for eng, lat in ((e256, z), (eC, zC)):
        lt = torch.from_numpy(lat).cuda().requires_grad_(True)
        pt = pts.clone().requires_grad_(True)
        y = functions.mlp_eval_autograd(eng, lt, pt, 0.1)
        (y * torch.linspace(-1, 1, y.numel(), device='cuda').reshape(-1, 1)).sum().backward()
        sdf, g = functions.mlp_grad(eng, lt.detach(), pts)
        small = functions.mlp_eval(eng, lt.detach(), pts[:100])          # the 16-ray tiles of a short point list
        torch.cuda.synchronize()
        out.append(dict(y=y.detach().cpu().numpy(), gl=lt.grad.cpu().numpy()[:, :min(C, 256)], gx=pt.grad.cpu().numpy(), sdf=sdf.cpu().numpy(),
                        g=g.cpu().numpy(), small=small.cpu().numpy()))
    _same(out[0], out[1], ('y', 'gl', 'gx', 'sdf', 'g', 'small'))


def test_embedding_batch_and_band_exact(pair):
    import torch
    from distr import binding, fixture, functions
    C, e256, eC, z, zC = pair
    H = W = 48
    K = fixture.make_intrinsic(H, W)
    cams = [fixture.make_camera(a, 15, 1.6, 0) for a in (0, 70, 140)]
    Rb = torch.from_numpy(np.stack([c[0] for c in cams])).cuda()
    Tb = torch.from_numpy(np.stack([c[1] for c in cams])).cuda()
    cfg = binding.make_cfg((H, W), K, march_step=24, buffer_size=3, marcher='pyramid_recursive', use_depth2normal=True)
    res = []
    for eng, code in ((e256, z), (eC, zC)):
        lat = torch.from_numpy(np.concatenate([np.asarray(code) * s for s in (1.0, 0.5, -1.0)])).cuda()
        with torch.no_grad():
            zb, mb, qb, db, nb = functions.render_batch_call(eng, cfg, lat, Rb, Tb)
            alone = [functions.render_call(eng, cfg, lat[i:i + 1], Rb[i], Tb[i]) for i in range(3)]
            band = functions.render_band_call(eng, cfg, lat[1:2], Rb[1], Tb[1], 16, 32)
        for i in range(3):       # per-view codes in one batch == the views alone
            assert torch.equal(zb[i], alone[i][0]) and torch.equal(mb[i], alone[i][1]) and torch.equal(nb[i], alone[i][4])
        assert torch.equal(band[0], alone[1][0].reshape(H, W)[16:32].reshape(-1)) and torch.equal(band[4], alone[1][4][16:32])
        res.append([t.cpu().numpy() for t in (zb, mb, qb, db, nb)])
    for x, y in zip(*res):
        assert np.array_equal(x, y)


def test_embedding_optimisation_exact(pair):
    """Five Adam iterations on the shape code: same losses and the same code (its tail stays zero)."""
    import torch
    from distr import fixture
    C, e256, eC, z, zC = pair
    H = W = 48
    K = fixture.make_intrinsic(H, W)
    R, T = fixture.make_camera(20, 25, 1.6, 0)
    codes, losses = [], []
    for eng, lat0 in ((e256, z), (eC, zC)):
        lat = torch.from_numpy(lat0 * 0.5).cuda().requires_grad_(True)
        opt = torch.optim.Adam([lat], lr=1e-2)
        Ls = []
        for _ in range(5):
            opt.zero_grad()
            a = helpers.hip_render(eng, H, W, K, R, T, lat.detach().cpu().numpy(), march_step=24, buffer_size=3, marcher='pyramid_recursive',
                                   use_depth2normal=True)
            lat.grad = torch.from_numpy(a['g_latent']).cuda()
            opt.step()
            Ls.append(a['loss'])
        losses.append(Ls)
        codes.append(lat.detach().cpu().numpy())
    m = min(C, 256)
    assert losses[0] == losses[1]
    assert np.array_equal(codes[0][:, :m], codes[1][:, :m]) and not np.any(codes[1][:, m:]) and not np.any(codes[0][:, m:])


@pytest.mark.parametrize('C', (64, 128, 300))
def test_dense_against_restatement(C):
    """Fixture decoder of code length C (every lin3 row and latent column non-zero) against the PyTorch restatement. (C = 508, one
    lin3 row, is covered bit for bit by the embedding tests; its fixture field is flat enough that min-|sdf| rows tie on ~0.1 % of
    pixels between the two summation orders.)"""
    import torch
    from distr import fixture, functions
    from oracle import torch_restatement as tr
    Ws, bs, latent = fixture.make_decoder_weights(latent_size=C)
    eng = functions.engine_from_weights(Ws, bs, 0)
    H = W = 72
    K = fixture.make_intrinsic(H, W)
    R, T = fixture.make_camera(40, 25, 1.6, 5)
    for marcher in ('pyramid_recursive', 'recursive', 'trivial'):
        kw = dict(march_step=30, buffer_size=3, use_depth2normal=True)
        a = helpers.hip_render(eng, H, W, K, R, T, latent, marcher=marcher, **kw)
        b = tr.render_fwd_bwd(Ws, bs, latent, H, W, K, R, T, helpers.loss_weights(H, W, 5), marcher=marcher, threads=16,
                              march_step=30, buffer_size=3, use_depth2normal=True)
        assert a['mask'].sum() > 50, marcher
        # min_sdf: a march decision next to a threshold (f32 GEMM against k-ordered chains, ~1e-7 apart) can pick another row on a few
        # pixels, like the mask flips compare() allows -- the same 0.1 % bar; the rest at 1e-4
        far = np.abs(a['min_sdf'].reshape(-1) - b['min_sdf'].reshape(-1)) > 1e-4
        assert int(far.sum()) <= max(1, int(0.001 * H * W)), (marcher, int(far.sum()))
        b = dict(b, min_sdf=np.where(far, a['min_sdf'].reshape(-1), b['min_sdf'].reshape(-1)))
        # a mask flip (<= 0.1 %, allowed by compare) moves the loss's support by a pixel: then the gradients carry that pixel's share
        # (~1 %), so the 1e-3 gradient bar applies when the masks agree and 2e-2 when they do not
        flips = int((a['mask'].reshape(-1) != b['mask'].reshape(-1)).sum())
        helpers.compare(a, b, H, W, tol_depth=1e-4, tol_grad=1e-3 if flips == 0 else 2e-2, normal_p99=max(1e-4, 1e-5 * float(K[0, 0])))
    # decode_sdf and its autograd against the restatement's decoder (float64)
    rs = np.random.RandomState(9)
    pts = ((rs.rand(4096, 3) - 0.5) * 1.6).astype(np.float32)
    lt = torch.from_numpy(latent).cuda().requires_grad_(True)
    pt = torch.from_numpy(pts).cuda().requires_grad_(True)
    y = functions.mlp_eval_autograd(eng, lt, pt)
    y.sum().backward()
    ref = tr.TorchRenderer(Ws, bs, H, W, K, dtype=torch.float64)
    l64 = torch.from_numpy(latent).double().requires_grad_(True)
    p64 = torch.from_numpy(pts).double().requires_grad_(True)
    y64 = ref.decode(l64, p64)
    y64.sum().backward()
    assert np.abs(y.detach().cpu().numpy().reshape(-1) - y64.detach().numpy()).max() <= 5e-6
    gx, gx64 = pt.grad.cpu().numpy(), p64.grad.numpy()
    gl, gl64 = lt.grad.cpu().numpy(), l64.grad.numpy()
    # point gradients: a pre-activation within f32 rounding of 0 takes the other ReLU branch on a few points (a kink, not an error)
    assert np.percentile(np.abs(gx - gx64), 99.9) <= 5e-6 * max(1.0, np.abs(gx64).max())
    assert np.abs(gl - gl64).max() <= 1e-3 * np.abs(gl64).max()


def test_load_decoder_code_length(tmp_path):
    """A DeepSDF experiment whose specs.json says CodeLength 128 loads and renders through the drop-in SDFRenderer."""
    import torch
    from core.sdfrenderer import SDFRenderer
    from core.utils.decoder_utils import load_decoder
    from distr import decoder_pack, fixture
    C = 128
    Ws, bs, latent = fixture.make_decoder_weights(latent_size=C)
    root = helpers.write_deepsdf_experiment(str(tmp_path / 'exp'), decoder_pack.fixture_state_dict(Ws, bs, True), '2000')
    specs = dict(helpers.DEEPSDF_SPECS, CodeLength=C)
    with open(os.path.join(root, 'specs.json'), 'w') as f:
        json.dump(specs, f)
    dec = load_decoder(root, '2000').cuda()
    size = 64
    K = fixture.make_intrinsic(size, size)
    R, T = fixture.make_camera(30, 20, 1.6, 0)
    ren = SDFRenderer(dec, K, img_hw=(size, size), march_step=30, buffer_size=3)
    lat, Rt, Tt = (torch.from_numpy(a).cuda() for a in (latent, R, T))
    with torch.no_grad():
        depth, mask = ren.render_depth(lat, Rt, Tt)[:2]
    assert int((mask.reshape(-1) > 0).sum()) > 100
    with pytest.raises(ValueError, match=r'\(1, 128\)'):
        ren.render_depth(lat[:, :64], Rt, Tt)
    with pytest.raises(decoder_pack.UnsupportedDecoder, match='code length'):
        SDFRenderer(dec, K, img_hw=(size, size), arith='bf16x6')


@pytest.mark.parametrize('C', (128, 300))
def test_split_arith_and_colour_refused(C):
    import torch
    from core.graph.deep_sdf_decoder import Decoder
    from core.sdfrenderer.renderer_rgb import SDFRenderer_color
    from distr import binding, decoder_pack, fixture, functions
    Ws, bs, latent = fixture.make_decoder_weights(latent_size=C)
    eng = functions.engine_from_weights(Ws, bs, 0)
    pts = torch.zeros(64, 3, device='cuda')
    lat = torch.from_numpy(latent).cuda()
    for arith in ('bf16x6', 'f16x3'):
        with pytest.raises(decoder_pack.UnsupportedDecoder, match='code length'):
            functions.mlp_eval(eng, lat, pts, arith=arith)
        cfg = binding.make_cfg((32, 32), fixture.make_intrinsic(32, 32), march_step=20, buffer_size=3, marcher='recursive', arith=arith)
        R, T = fixture.make_camera(0, 0, 1.6, 0)
        with pytest.raises(binding.DistrError, match='code length'):
            with torch.no_grad():
                functions.render_call(eng, cfg, lat, torch.from_numpy(R).cuda(), torch.from_numpy(T).cuda())
    dec = Decoder(C, [512] * 8, norm_layers=(), latent_in=[4])
    dec.load_state_dict({('lin%d.%s' % (l, n)): torch.from_numpy(a) for l, (W, b) in enumerate(zip(Ws, bs)) for n, a in (('weight', W), ('bias', b))})
    dec = dec.cuda()
    cWs, cbs, _ = fixture.make_color_decoder_weights()
    dcol = Decoder(256 + 256, [512, 512, 512, 512 + 256, 512, 512, 512, 512], norm_layers=(), latent_in=[4], last_dim=3)
    dcol.load_state_dict({('lin%d.%s' % (l, n)): torch.from_numpy(a) for l, (W, b) in enumerate(zip(cWs, cbs)) for n, a in (('weight', W), ('bias', b))})
    with pytest.raises(decoder_pack.UnsupportedDecoder, match='code length 256'):
        SDFRenderer_color(dec, dcol.cuda(), fixture.make_intrinsic(32, 32), img_hw=(32, 32))


def test_set_decoder_refuses_bad_code_length(fixture_decoder):
    """distr_set_decoder through ctypes: latent_size outside 1..508, or a buffer that does not fit its shapes, is refused."""
    import ctypes as Ct
    from distr import binding, decoder_pack, fixture
    ctx = binding.Context(0)
    Ws, bs, _ = fixture.make_decoder_weights(latent_size=300)
    flat = np.ascontiguousarray(decoder_pack.flatten(Ws, bs), dtype=np.float32)
    fp = flat.ctypes.data_as(Ct.POINTER(Ct.c_float))
    for nlat, n in ((0, flat.size), (509, flat.size), (128, flat.size), (300, flat.size - 1), (256, flat.size), (508, flat.size), (-1, flat.size)):
        desc = binding.DecoderDesc(latent_size=nlat, hidden=512, num_linear=9, latent_in=4)
        assert ctx.L.distr_set_decoder(ctx.h, Ct.byref(desc), fp, n) != 0, (nlat, n)
    ctx.set_decoder(flat, 300)                                   # the right description is accepted
    Ws1, bs1, _ = fixture.make_decoder_weights(latent_size=1)
    ctx.set_decoder(decoder_pack.flatten(Ws1, bs1), 1)
    ctx.set_decoder(decoder_pack.flatten(*fixture_decoder[:2]), 256)
