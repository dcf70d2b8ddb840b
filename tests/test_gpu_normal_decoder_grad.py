"""Normal-map losses through the decoder's second path on the GPU (normal_decoder_grad, include/distr_normal_grad.h).

The yardstick is fixed without a GPU by tests/test_normal_decoder_grad_host.py: the term restated in torch float64 as its definition and
as the closed form the kernels evaluate (tests/normal_grad_restatement.py), pinned to golden G27. Here: the HIP path against G27 itself,
against the closed form on the HIP render's own depths at the list sizes where the compaction and the segmented point list can go wrong,
byte equality of a batch with its stand-alone calls, byte equality with the parent behaviour when the option is off, a clamp that excludes
every surface sample, a wide decoder, and the full loss through SDFRenderer.render.
"""
import os

import numpy as np
import pytest

import helpers
import normal_grad_restatement as ngr
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

KEYS = ('g_latent', 'g_R', 'g_T')


@pytest.fixture(scope='module')
def f2():
    from distr import fixture
    return fixture.load_fixture_f2()


@pytest.fixture(scope='module')
def engine_f2(f2):
    from distr import functions
    return functions.engine_from_weights(f2[0], f2[1], 0)


@pytest.fixture(scope='module')
def dec_f1(fixture_decoder):
    return ngr.module(fixture_decoder[0], fixture_decoder[1])


def weights(B, H, W, seed):
    """Upstream gradient of the normal images of B views: view 0 = the goldens' w_n of that seed."""
    return np.stack([helpers.loss_weights(H, W, seed + v)[2] for v in range(B)])


def render(eng, cfg, latent, Rs, Ts, wn, option=None, flags=None):
    """B views through the one render node and a normal-only loss sum(normal * wn). option None: the keyword is not passed at all.
    Returns the forward outputs, the three gradients (one row per view; a shared code: one row) and, with the option's cfg qualifying,
    the term alone from the saved workspace (functions.normal_grad_term)."""
    import torch
    from distr import functions
    dev = eng.device
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev).requires_grad_(True)
    lat, R, T = t(latent), t(Rs), t(Ts)
    B = R.shape[0]
    kw = {} if option is None else dict(normal_decoder_grad=option)
    z, mask, q, depth, normal = functions.render_batch_call(eng, cfg, lat, R, T, flags, **kw)
    w = torch.from_numpy(wn).to(dev)
    out = dict(zdepth=z, mask=mask, min_sdf=q, depth=depth, normal=normal)
    node = normal.grad_fn
    if functions.normal_grad_applies(node.cfg):
        out['term'] = dict(zip(KEYS, (a.cpu().numpy() for a in functions.normal_grad_term(eng, node.cfg, node.ws, w, B, node.flags))))
    (normal * w).sum().backward()
    torch.cuda.synchronize()
    out = {k: (v.detach().cpu().numpy() if torch.is_tensor(v) else v) for k, v in out.items()}
    out.update(g_latent=lat.grad.cpu().numpy(), g_R=R.grad.cpu().numpy().reshape(B, 9), g_T=T.grad.cpu().numpy().reshape(B, 3))
    return out


def closed_form(dec, cfg_kw, H, W, K, a, v, latent, R, T, wn):
    """Restatement (b) of view v on the HIP render's own depths and mask."""
    S = ngr.Scene(H, W, K, a['zdepth'][v], a['mask'][v], wn[v], clamp_dist=cfg_kw.get('clamp_dist', 0.1), normalize=False,
                  transform_matrix=cfg_kw.get('transform_matrix'), use_transform=cfg_kw.get('use_transform', True))
    return ngr.closed_form(dec, S, latent, R, T)


def term_misses(got, ref, label):
    """HIP-vs-restatement bar for reduction-order differences: 1e-4 of each gradient's norm. Prints every figure,
    returns the components that miss."""
    bad = []
    for k in KEYS:
        r = np.asarray(ref[k], np.float64).reshape(-1)
        err, norm = float(np.abs(np.asarray(got[k], np.float64).reshape(-1) - r).max()), float(np.linalg.norm(r))
        print('%s %s: |err| %.3e  norm %.3e  ratio %.2e' % (label, k, err, norm, err / norm if norm else 0.0))
        if not err <= 1e-4 * norm:
            bad.append((label, k, err, norm))
    return bad


# ---- 1. golden G27, raw cases, with the option
def test_g27_raw_cases_with_the_option(engine, engine_f2, fixture_decoder, f2):
    """The reference's own gradients of a loss on the raw autograd normals alone: g_latent, g_R, g_T within max(2 x the golden's recorded
    floor, 2 x the float64 definition's residual against the golden) -- ngr.bar, fixed on the CPU -- with no allowance scaled by the full
    loss's gradient. Without the option the code and T get exactly zero (asserted: that is what the option is for)."""
    from distr import binding, fixture
    g = dict(np.load(os.path.join(GOLDEN, 'g27_normal_only_grad.npz')))
    H, W = int(g['H']), int(g['W'])
    wn = weights(1, H, W, int(g['loss_seed']))
    raw = [str(c) for c in g['cases'] if str(c).endswith('_raw')]
    assert len(raw) == 4
    for key in raw:
        fx, marcher = key.split('_', 1)[0], key.split('_', 1)[1].rsplit('_', 1)[0]
        eng, (Ws, bs, _) = (engine, fixture_decoder) if fx == 'f1' else (engine_f2, f2)
        assert fixture.weights_sha256(Ws, bs) == str(g[fx + '.weights_sha256'])
        cfg = binding.make_cfg((H, W), g['K'], march_step=int(g['march_step']), buffer_size=int(g['buffer_size']), ratio=float(g['ratio']),
                               marcher=marcher, use_depth2normal=False, normalize_normal=False)
        a = render(eng, cfg, g[fx + '.latent'], g['R'][None], g['T'][None], wn, option=True)
        assert int((a['mask'].reshape(H, W) != g[key + '.mask'].reshape(H, W)).sum()) == 0      # (mask flips: as the existing G27 test)
        for k in KEYS:
            ref = g['%s.%s' % (key, k)]
            err, bar = float(np.abs(a[k].reshape(ref.shape) - ref).max()), ngr.bar(g, key, k)
            print('%s %s: |ref| %.3e  HIP residual %.3e  bar %.3e' % (key, k, float(np.abs(ref).max()), err, bar))
            assert err <= bar, (key, k, err, bar)
        off = render(eng, cfg, g[fx + '.latent'], g['R'][None], g['T'][None], wn, option=False)
        assert not off['g_latent'].any() and not off['g_T'].any() and np.abs(a['g_latent']).max() > 1e-4


# ---- 2. HIP vs the closed form at the list sizes that matter
SIZE_CLASSES = (('none', 0, 0), ('below one tile', 1, 63), ('two tiles', 65, 127), ('several reduction blocks', 4097, 1 << 30))
# one image size (a batch shares it) and one camera position 1.5 units from the F1 blob: looking at it (the blob fills the image), panned
# by 40.6 and 41.2 degrees about its own centre (a sliver of the blob is left at the image border), and looking away. The term is
# proportional to f at the surface samples (|f| ~ 5e-6): the kernels evaluate that f in float64 (k_ng_f64), which is what
# lets float32 gradients meet a 1e-4 bar against the float64 restatement.
SIZE_PANS = (0.0, 40.6, 41.2, 180.0)


def size_views():
    import math
    from distr import fixture
    R0, T0 = fixture.make_camera(20, 15, 1.5, 5)
    Rs, Ts = [], []
    for deg in SIZE_PANS:
        a = math.radians(deg)
        Q = np.array([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]], np.float32)
        Rs.append((Q @ R0).astype(np.float32)); Ts.append((Q @ T0).astype(np.float32))      # x_cam = Q (R0 x + T0): the same camera position
    return np.stack(Rs), np.stack(Ts)


def test_term_matches_closed_form_at_every_list_size(engine, fixture_decoder, dec_f1):
    """Four views in one call whose valid-pixel counts are 0, within one 64-point tile, within two, and above 4096 (three blocks of the
    fixed-order compaction and of the camera sums, 64+ tiles of the segmented list): the term alone against restatement (b) on the HIP
    render's own depths."""
    from distr import binding, fixture
    H = W = 136
    K = fixture.make_intrinsic(H, W)
    Rs, Ts = size_views()
    kw = dict(march_step=100, buffer_size=3, marcher='recursive', use_depth2normal=False, normalize_normal=False)
    cfg = binding.make_cfg((H, W), K, **kw)
    wn = weights(4, H, W, 11)
    latent = fixture_decoder[2]
    a = render(engine, cfg, latent, Rs, Ts, wn, option=True)
    counts = [int(a['mask'][v].sum()) for v in range(4)]
    print('valid pixels per view:', counts)
    assert max(counts) > 2048, ('no view spans two blocks of the camera sums (2048 valid pixels each)', counts)
    for name, lo, hi in SIZE_CLASSES:
        assert any(lo <= c <= hi for c in counts), (name, counts)
    bad = []
    for v in range(4):
        b = closed_form(dec_f1, kw, H, W, K, a, v, latent, Rs[v], Ts[v], wn)
        assert b['n'] == counts[v]
        got = {k: a['term'][k][v] for k in KEYS}
        if counts[v] == 0:
            assert not any(got[k].any() for k in KEYS)
        else:
            bad += term_misses(got, b, 'view %d (%d px)' % (v, counts[v]))
    # a shared code: its gradient is the sum of the views' rows; code and T receive nothing else from a normal-only loss
    assert np.array_equal(a['g_latent'].reshape(-1), a['term']['g_latent'].sum(0, dtype=np.float32)) or \
        np.allclose(a['g_latent'].reshape(-1), a['term']['g_latent'].sum(0), rtol=0, atol=1e-6 * np.abs(a['term']['g_latent']).max())
    assert np.array_equal(a['g_T'], a['term']['g_T'])
    assert not bad, bad


# ---- 3. batch = stand-alone calls, byte for byte
def test_batch_views_equal_their_own_calls(engine, fixture_decoder):
    """Four views with own cameras and own codes in one call, one of them rendered with no_grad_camera, one without a valid pixel:
    every view's three outputs are byte-identical to its stand-alone call. The flagged view KEEPS this term's g_R and g_T: render()
    hands no_grad_camera to render_depth only (renderer.py:964), render_normal rebuilds the camera position and the rays from R and T
    with their gradients (renderer.py:881-882, called at :977 without the flag)."""
    from distr import binding, fixture
    H = W = 45
    K = fixture.make_intrinsic(H, W)
    cams = [fixture.make_camera(30, 20, 1.6, 10), fixture.make_camera(-60, 10, 1.9, 0), fixture.make_camera(20, 15, 1.6, 5), fixture.make_camera(140, -25, 1.4, 30)]
    Rs, Ts = np.stack([c[0] for c in cams]), np.stack([c[1] for c in cams])
    Ts[2] = -Ts[2]                                             # view 2 looks away: no valid pixel
    rs = np.random.RandomState(7)
    codes = (fixture_decoder[2] + 0.02 * rs.standard_normal((4, fixture_decoder[2].shape[1]))).astype(np.float32)
    cfg = binding.make_cfg((H, W), K, march_step=40, buffer_size=3, marcher='pyramid_recursive', use_depth2normal=False, normalize_normal=False)
    ALL = binding.VIEW_GRAD_DEPTH | binding.VIEW_GRAD_MASK | binding.VIEW_GRAD_CAMERA
    flags = [ALL, ALL & ~binding.VIEW_GRAD_CAMERA, ALL, ALL]
    wn = weights(4, H, W, 21)
    a = render(engine, cfg, codes, Rs, Ts, wn, option=True, flags=flags)
    counts = [int(a['mask'][v].sum()) for v in range(4)]
    print('valid pixels per view:', counts)
    assert counts[2] == 0 and min(counts[0], counts[1], counts[3]) > 64
    for v in range(4):
        s = render(engine, cfg, codes[v:v + 1], Rs[v:v + 1], Ts[v:v + 1], wn[v:v + 1], option=True, flags=flags[v:v + 1])
        for k in KEYS:
            assert np.array_equal(a['term'][k][v], s['term'][k][0]), (v, k)
            assert np.array_equal(a[k][v], s[k][0]), (v, k)
        for k in ('zdepth', 'mask', 'min_sdf', 'depth', 'normal'):
            assert np.array_equal(a[k][v], s[k][0]), (v, k)
    assert not any(a['term'][k][2].any() for k in KEYS)
    assert np.abs(a['term']['g_R'][1]).max() > 0 and np.abs(a['term']['g_T'][1]).max() > 0       # the flagged view keeps the term
    again = render(engine, cfg, codes, Rs, Ts, wn, option=True, flags=flags)                       # and the same bytes on every run
    for k in KEYS:
        assert np.array_equal(a['term'][k], again['term'][k]) and np.array_equal(a[k], again[k])


# ---- 4. option off = the parent's bytes
@pytest.mark.parametrize('mode', ['raw', 'unit', 'd2n'])
def test_option_off_and_inert_cases_are_byte_identical(engine, fixture_decoder, mode):
    """Outputs and gradients with normal_decoder_grad=False equal a call that does not pass the keyword, byte for byte; with the option on
    the forward outputs stay the same bytes in every case, and so do the gradients where the term is zero (unit normals) or absent
    (depth2normal)."""
    from distr import binding, fixture
    H = W = 48
    K = fixture.make_intrinsic(H, W)
    R, T = fixture.make_camera(30, 20, 1.6, 10)
    cfg = binding.make_cfg((H, W), K, march_step=30, buffer_size=3, marcher='pyramid_recursive', use_depth2normal=(mode == 'd2n'),
                           normalize_normal=(mode == 'unit'))
    wn = weights(1, H, W, 3)
    args = (engine, cfg, fixture_decoder[2], R[None], T[None], wn)
    plain, off, on = render(*args, option=None), render(*args, option=False), render(*args, option=True)
    assert int(plain['mask'].sum()) > 100
    for k in ('zdepth', 'mask', 'min_sdf', 'depth', 'normal'):
        assert np.array_equal(plain[k], off[k]) and np.array_equal(plain[k], on[k]), k
    for k in KEYS:
        assert np.array_equal(plain[k], off[k]), k
        if mode != 'raw':
            assert np.array_equal(plain[k], on[k]), k
    if mode == 'raw':
        assert np.abs(on['g_latent']).max() > 0 and not plain['g_latent'].any()
    if mode == 'unit':           # the entry point itself: zeros, no decoder work
        import torch
        from distr import functions
        lat, Rt, Tt = (torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(engine.device).requires_grad_(True) for x in (fixture_decoder[2], R[None], T[None]))
        normal = functions.render_batch_call(engine, cfg, lat, Rt, Tt)[4]
        out = functions.normal_grad_term(engine, normal.grad_fn.cfg, normal.grad_fn.ws, torch.from_numpy(wn), 1)
        assert all(not o.cpu().numpy().any() for o in out)


# ---- 5. a clamp that excludes the surface samples
def test_clamp_excludes_surface_samples(engine, fixture_decoder, dec_f1):
    """clamp_dist = 1e-7: the march cannot move, every ray inside the sphere stops where it entered (threshold 1: the first sample
    already counts as a hit), and every surface sample has |f| > clamp_dist -- the raw normal is zero there and so is the term, in the
    restatement and on the GPU."""
    from distr import binding, fixture
    H = W = 40
    K = fixture.make_intrinsic(H, W)
    R, T = fixture.make_camera(30, 20, 1.6, 10)
    kw = dict(march_step=12, buffer_size=3, marcher='pyramid_recursive', use_depth2normal=False, normalize_normal=False, clamp_dist=1e-7, threshold=1.0)
    cfg = binding.make_cfg((H, W), K, **kw)
    wn = weights(1, H, W, 9)
    a = render(engine, cfg, fixture_decoder[2], R[None], T[None], wn, option=True)
    n = int(a['mask'].sum())
    print('valid pixels:', n)
    assert n > 100
    b = closed_form(dec_f1, kw, H, W, K, a, 0, fixture_decoder[2], R, T, wn)
    assert b['n'] == n and not any(np.asarray(b[k]).any() for k in KEYS)
    assert not any(a['term'][k].any() for k in KEYS) and not a['normal'].any()


# ---- 6. a wide decoder
def test_wide_decoder_equals_its_embedding(fixture_decoder):
    """The C = 256 fixture embedded into C = 64 (tests/test_gpu_code_length.py): the wide layout's point-list backward gives the term of
    the C = 256 decoder on the embedded coordinates, at the bar of test 2."""
    from distr import binding, fixture, functions
    from test_gpu_code_length import _embedding_wide
    (W256, b256), (WC, bC), z256, zC = _embedding_wide(fixture_decoder, 64)
    e256, eC = functions.engine_from_weights(W256, b256, 0), functions.engine_from_weights(WC, bC, 0)
    assert eC.latent_size == 64
    H = W = 64
    K = fixture.make_intrinsic(H, W)
    R, T = fixture.make_camera(35, 20, 1.6, 10)
    cfg = binding.make_cfg((H, W), K, march_step=30, buffer_size=3, marcher='recursive', use_depth2normal=False, normalize_normal=False)
    wn = weights(1, H, W, 13)
    a = render(e256, cfg, z256, R[None], T[None], wn, option=True)
    b = render(eC, cfg, zC, R[None], T[None], wn, option=True)
    assert int(a['mask'].sum()) > 150 and np.array_equal(a['mask'], b['mask'])
    assert b['term']['g_latent'].shape == (1, 64) and np.abs(b['term']['g_latent']).max() > 0
    ref = dict(g_latent=a['term']['g_latent'][:, :64], g_R=a['term']['g_R'], g_T=a['term']['g_T'])
    assert not term_misses({k: b['term'][k] for k in KEYS}, ref, 'C = 64 vs C = 256')
    assert not a['term']['g_latent'][:, 64:].any()


# ---- 7. the full loss through SDFRenderer.render
def test_full_loss_is_option_off_plus_the_term(fixture_decoder):
    """Depth + normal + silhouette loss through SDFRenderer(..., normal_decoder_grad=True).render(...).backward(): the option-off gradient
    plus the term of a normal-only backward, to 1e-6 of each gradient's size (one float32 addition apart)."""
    import torch
    from core.graph.deep_sdf_decoder import Decoder
    from core.sdfrenderer.renderer import SDFRenderer
    from distr import fixture
    Ws, bs, latent = fixture_decoder
    dec = Decoder(256, [512] * 8, norm_layers=(), latent_in=[4])
    dec.load_state_dict({('lin%d.%s' % (l, n)): torch.from_numpy(a) for l, (W_, b) in enumerate(zip(Ws, bs)) for n, a in (('weight', W_), ('bias', b))})
    dec = dec.cuda().eval()
    H = W = 48
    K = fixture.make_intrinsic(H, W)
    R, T = fixture.make_camera(30, 20, 1.6, 10)
    wd, wq, wn = (torch.from_numpy(a).cuda() for a in helpers.loss_weights(H, W, 5))

    def run(option, full=True, normal=True):
        r = SDFRenderer(dec, K, img_hw=(H, W), march_step=30, buffer_size=3, normal_decoder_grad=option)
        assert r.normal_decoder_grad is option
        lat, Rt, Tt = (torch.from_numpy(x).cuda().requires_grad_(True) for x in (latent, R, T))
        depth, nrm, mask, q = r.render(lat, Rt, Tt, normalize_normal=False)
        L = (nrm * wn).sum() if normal else 0.0
        if full:
            L = L + (depth * wd)[mask.bool()].sum() + (q * wq).sum()
        L.backward()
        return [t.grad.double().cpu().numpy() for t in (lat, Rt, Tt)], (depth.detach(), nrm.detach(), mask, q.detach())

    on, out_on = run(True)
    off, out_off = run(False)
    n_on, _ = run(True, full=False)
    n_off, _ = run(False, full=False)
    assert all(torch.equal(x, y) for x, y in zip(out_on, out_off)) and int(out_on[2].sum()) > 100
    for k, a, b, t1, t0 in zip(KEYS, on, off, n_on, n_off):
        term = t1 - t0                                         # the term of the normal-only backward
        err, scale = float(np.abs(a - (b + term)).max()), float(np.abs(a).max())
        print('%s: |full on - (full off + term)| %.3e of %.3e; |term| %.3e' % (k, err, scale, float(np.abs(term).max())))
        assert err <= 1e-6 * scale, (k, err, scale)
    assert np.abs(n_on[0]).max() > 0 and not n_off[0].any()
