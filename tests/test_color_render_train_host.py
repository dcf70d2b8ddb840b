"""CPU-only checks of the colour decoder's weight gradients through the colour render: the plan that cuts the
views' lists into train calls of the colour net (out_dim = 3), the new part of the C ABI (include/distr_color_train.h) against the
binding and the library, its refusals on a context without a device, and the refusals of the Python layer."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from conftest import ROOT

K = np.array([[44., 0, 20], [0, 46., 24], [0, 0, 1]])


# ------------------------------------------------------------------------------------------------ the plan of the train calls
def _check_plan(counts, limit, out_dim):
    from distr import binding, functions
    plan = functions.render_train_chunks(counts, limit, out_dim=out_dim)
    assert plan == functions.render_train_chunks(list(counts), limit, out_dim)        # a function of its arguments alone
    seen = [[] for _ in counts]
    last = (-1, -1)
    for piece in plan:
        assert 1 <= len(piece) <= binding.MAX_SEGMENTS
        assert functions.train_plan_bytes([n for _, _, n in piece], out_dim) <= limit
        for v, a, n in piece:
            assert n > 0 and a % 64 == 0 and a + n <= counts[v]
            assert (v, a) > last                                                  # view order, then row order
            last = (v, a)
            seen[v].append((a, n))
    for v, c in enumerate(counts):                                                # every row exactly once, no gap
        at = 0
        for a, n in seen[v]:
            assert a == at
            at += n
        assert at == c
    return plan


def test_chunks_of_the_colour_net_cover_every_row_once():
    from distr import functions
    big = 1 << 40
    assert functions.render_train_chunks([], big, out_dim=3) == [] and functions.render_train_chunks([0, 0], big, out_dim=3) == []
    assert _check_plan([1920], big, 3) == [[(0, 0, 1920)]]
    assert _check_plan([5, 0, 64, 0, 65], big, 3) == [[(0, 0, 5), (2, 0, 64), (4, 0, 65)]]     # empty views get no segment
    # the three per-row arrays z, tanh, dz have three floats per row: a limit that holds exactly 256 rows of the colour net
    assert functions.train_plan_bytes([256], 3) > functions.train_plan_bytes([256], 1)
    lim = functions.train_plan_bytes([256], 3)
    plan = _check_plan([1000], lim, 3)
    assert [p[0][1:] for p in plan] == [(0, 256), (256, 256), (512, 256), (768, 232)]
    # the three ways to ask for the SDF net's plan agree
    assert functions.render_train_chunks([1000], lim) == functions.render_train_chunks([1000], lim, 1) == functions.render_train_chunks([1000], lim, out_dim=1)
    plan = _check_plan([100, 0, 300, 64, 7], functions.train_plan_bytes([128, 128], 3), 3)
    assert len(plan) >= 3 and any(len(p) > 1 for p in plan) and any(a > 0 for p in plan for _, a, _ in p)
    plan = _check_plan([3] * 150, big, 3)
    assert [len(p) for p in plan] == [64, 64, 22]
    rs = np.random.RandomState(35)
    for _ in range(20):
        counts = [int(c) for c in rs.choice([0, 1, 63, 64, 65, 200, 1000, 5000], rs.randint(1, 9))]
        _check_plan(counts, functions.train_plan_bytes([int(rs.choice([64, 128, 640, 4096]))] * int(rs.randint(1, 3)), 3), 3)
    with pytest.raises(ValueError, match='do not hold one tile'):
        functions.render_train_chunks([10], functions.train_plan_bytes([64], 3) - 1, out_dim=3)
    with pytest.raises(ValueError):
        functions.render_train_chunks([10, -1], big, out_dim=3)


def test_out_dim_1_plans_are_unchanged():
    """The default keeps every existing plan: the plans test_render_train_host.py pins, with and without the argument."""
    from distr import functions
    big = 1 << 40
    lim = functions.train_plan_bytes([256])
    for counts, limit in (([2708], big), ([5, 0, 64, 0, 65], big), ([1000], lim), ([100, 0, 300, 64, 7], functions.train_plan_bytes([128, 128])), ([3] * 150, big)):
        assert functions.render_train_chunks(counts, limit) == functions.render_train_chunks(counts, limit, out_dim=1)
    assert [p[0][1:] for p in functions.render_train_chunks([1000], lim)] == [(0, 256), (256, 256), (512, 256), (768, 232)]
    # a limit between the two nets' needs: the SDF net's 256 rows fit, the colour net's do not
    assert [p[0][2] for p in functions.render_train_chunks([256], lim)] == [256]
    cut = [p[0][2] for p in functions.render_train_chunks([256], lim, out_dim=3)]
    assert len(cut) > 1 and sum(cut) == 256 and all(n % 64 == 0 for n in cut), cut


# ------------------------------------------------------------------------------------------------ header, binding, library
def test_color_train_abi_declared_exported_and_checked():
    from distr import binding
    hdr = open(os.path.join(ROOT, 'include', 'distr_color_train.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    assert set(re.findall(r'\b(distr_[a-z0-9_]+)\s*\(', hdr)) == set(binding.COLOR_TRAIN_EXPORTS)
    top = open(os.path.join(ROOT, 'include', 'distr.h')).read()
    assert '#include "distr_color_train.h"' in top and 'distr_color_train.h' in binding.HEADERS
    assert 'DISTR_ABI_VERSION 6u' in top and binding.ABI_VERSION == 6
    binding.build_library()
    L = binding.lib()
    for name in binding.COLOR_TRAIN_EXPORTS:
        assert hasattr(L, name), name
    assert int(L.distr_abi_version()) == 6
    assert len(L.distr_color_stage_samples_export_batch.argtypes) == 13           # the header's thirteen parameters


def test_export_refusals_without_a_device():
    """The checks of distr_color_stage_samples_export_batch are host code: a context created without a device still answers them."""
    from distr import binding
    binding.build_library()
    L = binding.lib()
    H, W = 48, 40
    P = H * W
    cfg = binding.make_cfg((H, W), K, march_step=24, buffer_size=3, marcher='recursive')
    h = C.c_void_p()
    L.distr_create_abi(C.byref(h), 0, binding.ABI_VERSION)                   # (fails for lack of a device; the context still answers)
    fwd, bwd = C.c_size_t(), C.c_size_t()
    assert L.distr_color_stage_workspace_bytes(h, C.byref(cfg), 1, C.byref(fwd), C.byref(bwd)) == 0 and fwd.value > 0 and bwd.value > 0
    f2, b2 = C.c_size_t(), C.c_size_t()
    assert L.distr_color_stage_workspace_bytes(h, C.byref(cfg), 2, C.byref(f2), C.byref(b2)) == 0
    p = C.c_void_p(4096)                                                     # never dereferenced: every call below is refused before a launch
    INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -4

    def call(c=cfg, nviews=1, ws=p, ws_bytes=None, wb=p, wb_bytes=None, xyz=p, up=p, index=None, cap=P, counts=p):
        return L.distr_color_stage_samples_export_batch(h, C.byref(c), nviews, ws, fwd.value if ws_bytes is None else ws_bytes, wb,
                                                        bwd.value if wb_bytes is None else wb_bytes, xyz, up, index, cap, counts, None)
    assert L.distr_color_stage_samples_export_batch(None, C.byref(cfg), 1, p, fwd.value, p, bwd.value, p, p, None, P, p, None) == INVALID
    for kw in (dict(ws=None), dict(wb=None), dict(xyz=None), dict(up=None), dict(counts=None)):
        assert call(**kw) == INVALID and b'null' in L.distr_last_error(h), kw
    assert call(cap=P - 1) == INVALID and b'cap' in L.distr_last_error(h)
    assert call(cap=0) == INVALID and call(cap=-1) == INVALID
    assert call(nviews=0) == INVALID and call(nviews=65) == INVALID and b'nviews' in L.distr_last_error(h)
    bad = cfg.clone()
    bad.struct_size -= 4
    assert call(c=bad) == INVALID and b'struct_size' in L.distr_last_error(h)
    band = binding.make_cfg((H, W), K, march_step=24, buffer_size=3, marcher='recursive', band=(8, 16))
    assert call(c=band) == UNSUPPORTED and b'row bands' in L.distr_last_error(h)      # as the stage refuses them
    assert L.distr_color_stage_workspace_bytes(h, C.byref(band), 1, C.byref(f2), C.byref(b2)) == UNSUPPORTED
    assert call(ws_bytes=fwd.value - 1) == WORKSPACE and b'forward workspace' in L.distr_last_error(h)
    assert call(wb_bytes=bwd.value - 1) == WORKSPACE and b'backward workspace' in L.distr_last_error(h)
    assert call(nviews=2) == WORKSPACE                                       # the sizes of one view do not hold two
    L.distr_destroy(h)


# ------------------------------------------------------------------------------------------------ the Python layer
def test_refusals_of_the_python_layer():
    """What is refused before anything reaches a device, each with its reason."""
    import torch
    from distr import binding, functions
    cfg = binding.make_cfg((48, 40), K, march_step=24, buffer_size=3, marcher='recursive')
    w = [torch.zeros(1, requires_grad=True) for _ in range(18)]
    z = torch.zeros(1)
    with pytest.raises(ValueError, match='18 tensors, got 17'):
        functions.color_stage_call(None, cfg, z, z, z, z, z, z, weights=w[:17])
    with pytest.raises(ValueError, match='18 tensors, got 17'):
        functions.color_stage_weight_grads(None, cfg, {}, None, w[:17])
    band = binding.make_cfg((48, 40), K, march_step=24, buffer_size=3, marcher='recursive', band=(8, 16))
    with pytest.raises(NotImplementedError, match='row bands'):
        functions.color_stage_call(None, band, z, z, z, z, z, z, weights=w)
    with pytest.raises(ValueError, match='lighting_locations requires grad'):
        functions.color_lights(torch.device('cpu'), 1, torch.zeros(1, 3, requires_grad=True), None)
    with pytest.raises(ValueError, match='lighting_energies requires grad'):
        functions.color_lights(torch.device('cpu'), 1, torch.zeros(1, 3), torch.ones(1, requires_grad=True))
    assert functions.color_train_net([torch.zeros(512, 256 + 32 + 3)]) == (288, 253, 3)


def test_the_public_flag_exists():
    """SDFRenderer_color(..., color_decoder_grad=True): the keyword is taken (default off). Without a GPU the constructor ends where it
    always did, at the device check of SDFRenderer -- not at the keyword."""
    import torch
    from core.graph.deep_sdf_decoder import Decoder
    from core.sdfrenderer import SDFRenderer_color
    from distr import fixture
    sig = inspect.signature(SDFRenderer_color.__init__)
    assert sig.parameters['color_decoder_grad'].default is False
    dims_c = [512] * 8
    dims_c[3] += 32
    dec, dec_c = Decoder(256, [512] * 8, latent_in=[4]), Decoder(288, dims_c, latent_in=[4], last_dim=3)
    args = (fixture.make_intrinsic(32, 32),)
    if not torch.cuda.is_available():
        with pytest.raises(ValueError, match='No GPU device found'):
            SDFRenderer_color(dec, dec_c, *args, img_hw=(32, 32), color_decoder_grad=True)
        return
    r = SDFRenderer_color(dec.cuda(), dec_c.cuda(), *args, img_hw=(32, 32), color_decoder_grad=True)
    assert r.color_decoder_grad is True
    assert SDFRenderer_color(dec, dec_c, *args, img_hw=(32, 32)).color_decoder_grad is False


# ------------------------------------------------------------------------------------------------ golden G35: the CPU chain, the loss
G35 = os.path.join(ROOT, 'tests', 'golden', 'g35_color_render_weight_grad.npz')


@pytest.fixture(scope='module')
def g35():
    return dict(np.load(G35))


def test_g35_is_complete_and_small(g35, fixture_decoder):
    import color_render_train_restatement as crt
    from distr import fixture
    assert os.path.getsize(G35) < 600 << 10
    Wc, bc, code = fixture.make_color_decoder_weights(color_size=int(g35['color_size']))
    assert str(g35['weights_sha256']) == fixture.weights_sha256(*fixture_decoder[:2]) and str(g35['color_weights_sha256']) == fixture.weights_sha256(Wc, bc)
    assert np.array_equal(g35['color_code'], code) and np.array_equal(g35['latent'], fixture_decoder[2])
    assert sorted(str(c) for c in g35['case_names']) == sorted(crt.CASES) and int(g35['noise_draws']) >= 3 and g35['lights'].shape == (1, 3)
    for case in crt.CASES:
        names = [k[len(case) + 1:] for k in g35 if k.startswith(case + '_g_')]
        want = ['g_color_code', 'g_latent', 'g_R', 'g_T', 'g_lin8_weight'] + ['g_bias%d' % l for l in range(9)]
        mats = ['g_v%d' % l for l in range(8)] if case == 'wn' else ['g_W%d' % l for l in range(8)]
        want += [m + s for m in mats for s in ('_rowsum', '_colsum', '_rows')] + (['g_weight_g%d' % l for l in range(8)] if case == 'wn' else [])
        assert sorted(names) == sorted(want), case
        for k in names + list(crt.VALUES):
            assert np.abs(g35['%s_%s' % (case, k)]).max() > 0 and 0 <= float(g35['%s_floor_%s' % (case, k)]) < 0.1, (case, k)
        m, gm = g35[case + '_mask'] != 0, g35['gt_mask'] != 0
        assert m.sum() > 100 and 0 < (m & gm).sum() < min(m.sum(), gm.sum()) and int(g35[case + '_num_rows']) == m.sum()
    for i, (h, w) in enumerate(crt.SSIM_PAIRS):
        assert g35['ssim%d_x' % i].shape == g35['ssim%d_y' % i].shape == g35['ssim%d_g' % i].shape == (3, h, w) and g35['ssim%d_g' % i].dtype == np.float32


@pytest.mark.parametrize('case', ['unlit', 'lit', 'wn'])
def test_cpu_chain_matches_the_reference(g35, orc, cpu_oracle, case):
    """The oracle's render + the colour stage in float64 + the list (points, g_rgb * s) under color_train_restatement.gradients against the
    reference's own backward with the colour decoder's parameters requiring grad: the oracle's mask equals the reference's, and every
    recorded quantity is inside max(1e-3, 2 x its floor). This pins the decomposition the GPU path implements to the reference."""
    import color_render_train_restatement as crt
    from distr import fixture
    Wc, bc, _ = fixture.make_color_decoder_weights(color_size=int(g35['color_size']))
    sd = crt.wn_state_dict(g35, Wc, bc) if crt.CASES[case][1] else None
    got, mask, n = crt.chain(cpu_oracle, orc, case, Wc, bc, sd, g35['latent'], g35['color_code'], g35['R'], g35['T'], g35[case + '_gt'], g35['gt_mask'],
                             g35['lights'], g35['energies'])
    assert int((mask != (g35[case + '_mask'] != 0)).sum()) == 0 and n == int(g35[case + '_num_rows'])
    res = crt.residuals(got, g35, case)
    print(case, '%d rows;' % n, ', '.join('%s %.1e' % (k, r) for k, r, _ in res))
    bad = [(k, r, bar) for k, r, bar in res if not r <= bar]
    assert not bad, (case, bad)


def _loss_cases():
    """Image pairs and masks of the loss tests: the sizes of the GPU tests, masks touching every border, an empty overlap."""
    rs = np.random.RandomState(352)
    out = []
    for h, w in ((1, 1), (1, 5), (3, 3), (16, 16), (1, 257), (17, 19)):
        rgb, gt = rs.rand(h, w, 3), rs.rand(h, w, 3)
        full = np.ones((h, w), bool)
        out.append((rgb, full, gt, full))
        if h * w > 1:
            out.append((rgb, rs.rand(h, w) < 0.7, gt, rs.rand(h, w) < 0.7))
    out.append((rs.rand(5, 7, 3), np.arange(35).reshape(5, 7) % 2 == 0, rs.rand(5, 7, 3), np.arange(35).reshape(5, 7) % 2 == 1))     # empty overlap
    return out


def test_loss_restatement_against_float64_autograd():
    """tests/color_loss_restatement.py (numpy, the gradient by hand) against autograd through the float64 torch composition of the same
    formula: values and gradients to 1e-12 -- of the gradient's largest entry, which is 1 / (3 N) for the L1 term."""
    import torch
    import color_loss_restatement as clr
    worst = 0.0
    for rgb, m, gt, gm in _loss_cases():
        got = clr.color_loss(rgb, m, gt, gm)
        assert got['overlap'] == int((m & gm).sum())
        t = torch.tensor(rgb, dtype=torch.float64, requires_grad=True)
        l1, ssim = clr.torch_color_loss(t, torch.as_tensor(m), torch.tensor(gt, dtype=torch.float64), torch.as_tensor(gm))
        g_ssim, = torch.autograd.grad(ssim, t, retain_graph=True)
        assert abs(got['ssim'] - ssim.item()) <= 1e-12
        top = max(g_ssim.abs().max().item(), 1e-300)
        worst = max(worst, np.abs(got['g_ssim'] - g_ssim.numpy()).max() / top)
        if got['overlap']:
            g_l1, = torch.autograd.grad(l1, t)
            assert abs(got['l1'] - l1.item()) <= 1e-12 and np.abs(got['g_l1'] - g_l1.numpy()).max() <= 1e-12 * g_l1.abs().max().item()
        else:                                   # the one divergence from the reference: 0 and a zero gradient, not NaN
            assert got['l1'] == 0.0 and not got['g_l1'].any() and not np.isfinite(l1.item())
    print('ssim gradient: worst distance from float64 autograd %.2e of the largest entry' % worst)
    assert worst <= 1e-12


def test_clamp_edge_of_the_ssim_loss():
    """In exact arithmetic ssim is a product of two ratios in [-1, 1], so (1 - ssim) / 2 never leaves [0, 1]: the clamp binds only where
    rounding carries a value across its edge. An image pair whose ssim is below -1 + 1e-4 in every interior window (zero window means,
    y = -x, a large variance against C2) sits on that edge: the restatement and float64 autograd agree there, and the GPU test runs the
    fused loss on it."""
    import torch
    import color_loss_restatement as clr
    x, y = clamp_pair()
    loss, g, s = clr.ssim_loss(x, y)
    assert (s[:, 1:-1, 1:-1] < -1.0 + 1e-4).all() and (s >= -1.0).all() and (s > -0.9).any()
    t = torch.tensor(y, requires_grad=True)
    ov = torch.ones(x.shape[1:], dtype=torch.bool)
    _, ssim = clr.torch_color_loss(t.permute(1, 2, 0), ov, torch.tensor(x).permute(1, 2, 0), ov)
    g64, = torch.autograd.grad(ssim, t)
    # (the gradient is what is left of terms near 1e-3 that cancel to 2e-7: the bar is absolute here)
    assert abs(loss - ssim.item()) <= 1e-12 and np.abs(g - g64.numpy()).max() <= 1e-12 and g64.abs().max().item() > 1e-8


def clamp_pair(h=6, w=9):
    """(x, y) (3, h, w) float64: vertical stripes (a, -a, 0) -- every interior 3 x 3 window has mean zero -- and the negative image."""
    stripe = np.tile(np.array([1.0, -1.0, 0.0]), w // 3 + 1)[:w]
    x = np.stack([np.tile(4.0 * (c + 1) * stripe, (h, 1)) for c in range(3)])
    return x, -x


def test_ssim_records_of_the_reference(g35):
    """The reference's f32 loss_ssim and its gradient on three raw image pairs against the float64 restatement: the distance is the f32
    error of the reference's own evaluation (sigma = E[x^2] - mu^2 cancels against C2 = 9e-4), and twice it is the bar the fused loss is
    held to. Printed here (and written in DESIGN.md section 8j); asserted only to be what f32 rounding can explain: below 1e-4 of the
    gradient's largest entry and 1e-6 for the value."""
    import color_loss_restatement as clr
    import color_render_train_restatement as crt
    for i, (h, w) in enumerate(crt.SSIM_PAIRS):
        loss, g, _ = clr.ssim_loss(g35['ssim%d_x' % i], g35['ssim%d_y' % i])
        dv = abs(float(g35['ssim%d_loss' % i]) - loss)
        dg = float(np.abs(g35['ssim%d_g' % i] - g).max() / np.abs(g).max())
        print('loss_ssim record %d x %d: value %.3e from float64, gradient %.3e of its largest entry' % (h, w, dv, dg))
        assert dv <= 1e-6 and dg <= 1e-4


def test_loss_refusals_without_a_device():
    """The checks of distr_color_loss_forward_batch / _backward_batch are host code; the workspace sizes are a function of the sizes alone."""
    from distr import binding
    binding.build_library()
    L = binding.lib()
    size = L.distr_color_loss_workspace_bytes
    assert size(16, 16, 1, 0) == 1 * 3 * 4 + 256 and size(17, 19, 3, 0) == 3 * 2 * 3 * 4 + 256 and size(17, 19, 3, 1) == 3 * 323 * 9 * 4 + 256
    assert size(0, 5, 1, 0) == 0 and size(5, 0, 1, 1) == 0 and size(5, 5, 0, 0) == 0 and size(5, 5, 65, 0) == 0 and size(4096, 4097, 1, 0) == 0
    assert size(4096, 4096, 1, 0) > 0
    h = C.c_void_p()
    L.distr_create_abi(C.byref(h), 0, binding.ABI_VERSION)                   # (fails for lack of a device; the context still answers)
    p = C.c_void_p(4096)                                                     # never dereferenced
    INVALID, WORKSPACE = -1, -4
    fb, bb = size(5, 7, 2, 0), size(5, 7, 2, 1)

    def fwd(H=5, W=7, B=2, rgb=p, m=p, gt=p, gm=p, want=1, l1=p, ssim=p, ov=p, ws=p, n=fb):
        return L.distr_color_loss_forward_batch(h, H, W, B, rgb, m, gt, gm, want, l1, ssim, ov, ws, n, None)

    def bwd(H=5, W=7, B=2, rgb=p, m=p, gt=p, gm=p, ov=p, g1=p, g2=p, out=p, ws=p, n=bb):
        return L.distr_color_loss_backward_batch(h, H, W, B, rgb, m, gt, gm, ov, g1, g2, out, ws, n, None)
    assert L.distr_color_loss_forward_batch(None, 5, 7, 2, p, p, p, p, 1, p, p, p, p, fb, None) == INVALID
    assert L.distr_color_loss_backward_batch(None, 5, 7, 2, p, p, p, p, p, p, p, p, p, bb, None) == INVALID
    for kw in (dict(rgb=None), dict(m=None), dict(gt=None), dict(gm=None), dict(l1=None), dict(ov=None), dict(ssim=None)):
        assert fwd(**kw) == INVALID and b'null' in L.distr_last_error(h), kw
    for kw in (dict(rgb=None), dict(m=None), dict(gt=None), dict(gm=None), dict(ov=None), dict(out=None)):
        assert bwd(**kw) == INVALID and b'null' in L.distr_last_error(h), kw
    for f in (fwd, bwd):
        assert f(H=0) == INVALID and b'image size' in L.distr_last_error(h)
        assert f(H=4096, W=4097) == INVALID
        assert f(B=0) == INVALID and f(B=65) == INVALID and b'nviews' in L.distr_last_error(h)
        assert f(ws=None) == WORKSPACE and b'workspace' in L.distr_last_error(h)
    assert fwd(n=fb - 1) == WORKSPACE and b'forward workspace' in L.distr_last_error(h)
    assert bwd(n=bb - 1) == WORKSPACE and b'backward workspace' in L.distr_last_error(h)
    L.distr_destroy(h)


def test_color_gt_is_an_observation():
    import torch
    from core.utils.loss_utils import compute_loss_color_batch
    z = torch.zeros(1, 3, 3, 3)
    with pytest.raises(ValueError, match='color_gt requires grad'):
        compute_loss_color_batch(z, torch.ones(1, 3, 3), z.clone().requires_grad_(True), torch.ones(1, 3, 3))
    with pytest.raises(RuntimeError, match='must be on the GPU'):
        compute_loss_color_batch(z, torch.ones(1, 3, 3), z, torch.ones(1, 3, 3))
