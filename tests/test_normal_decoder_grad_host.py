"""CPU-only checks of the normal-map loss's decoder-path gradient (include/distr_normal_grad.h).

The yardstick first: the term restated in torch float64 (tests/normal_grad_restatement.py) as its DEFINITION (double backward through the
torch Decoder) and as the CLOSED FORM the kernels evaluate, on the surface depths and masks of the CPU oracle's render of golden G27's
configuration (64 x 64, 20 steps, buffer 3, fixtures F1 and F2, recursive / pyramid_recursive), against the gradients the reference
itself returned (tests/golden/g27_normal_only_grad.npz). Then the host side of the C ABI: workspace sizes and refusals.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import helpers
import normal_grad_restatement as ngr
from conftest import GOLDEN, ROOT

G27 = os.path.join(GOLDEN, 'g27_normal_only_grad.npz')
KEYS = ('g_latent', 'g_R', 'g_T')


def g27_cases():
    g = dict(np.load(G27))
    return g, [str(c) for c in g['cases']]


bar = ngr.bar


@pytest.fixture(scope='module')
def restated(fixture_decoder, orc):
    """Per G27 case: (definition, closed form) on the oracle's render. Computed once, never modified."""
    from distr import fixture
    g, cases = g27_cases()
    H, W = int(g['H']), int(g['W'])
    _, _, wn = helpers.loss_weights(H, W, int(g['loss_seed']))
    out = {}
    for fx, (Ws, bs, _) in (('f1', fixture_decoder), ('f2', fixture.load_fixture_f2())):
        assert fixture.weights_sha256(Ws, bs) == str(g[fx + '.weights_sha256'])
        O, dec = orc.Oracle(Ws, bs), ngr.module(Ws, bs)
        for key in [c for c in cases if c.startswith(fx)]:
            marcher, mode = key.split('_', 1)[1].rsplit('_', 1)
            kw = dict(march_step=int(g['march_step']), buffer_size=int(g['buffer_size']), ratio=float(g['ratio']), marcher=marcher,
                      use_depth2normal=False, normalize_normal=(mode == 'unit'))
            r = O.render(orc.make_cfg(H, W, g['K'], **kw), g[fx + '.latent'], g['R'], g['T'])
            assert int((r['mask'].reshape(H, W) != g[key + '.mask'].reshape(H, W)).sum()) == 0, key
            S = ngr.Scene(H, W, g['K'], r['zdepth'], r['mask'], wn, clamp_dist=0.1, normalize=(mode == 'unit'))
            out[key] = (ngr.definition(dec, S, g[fx + '.latent'], g['R'], g['T']), ngr.closed_form(dec, S, g[fx + '.latent'], g['R'], g['T']))
    return g, out


def test_definition_matches_the_reference_golden_raw(restated):
    """(a) against G27's four *_raw cases within 2 x the recorded floor, or within its own recorded residual (tests/normal_grad_restatement.py
    RESIDUAL_A: float64 on the oracle's depths against the reference's float32; worst 2.5 % of a gradient, f2_recursive g_latent); g_R
    after adding the share of the explicit `R @ normal` product."""
    g, out = restated
    raw = [k for k in out if k.endswith('_raw')]
    assert len(raw) == 4
    for key in raw:
        a = out[key][0]
        assert a['n'] > 150
        got = dict(g_latent=a['g_latent'], g_R=a['g_R'] + a['g_R_product'], g_T=a['g_T'])
        for k in KEYS:
            ref = g['%s.%s' % (key, k)]
            err = float(np.abs(got[k].reshape(ref.shape) - ref).max())
            floor2, rec = 2.0 * float(g['%s.%s_floor' % (key, k)]), ngr.RESIDUAL_A[key][k]
            print('%s %s: |ref| %.3e  (a) residual %.3e  2 x floor %.3e  recorded residual %.3e' % (key, k, float(np.abs(ref).max()), err, floor2, rec))
            # within 2 x floor, or -- float64 against the reference's float32 -- the residual recorded in RESIDUAL_A (which then sets the
            # component's bar, ngr.bar), never more than 3 % of the gradient
            assert err <= max(floor2, 1.25 * rec) and err <= 0.03 * float(np.abs(ref).max()), (key, k, err, floor2, rec)
            assert bar(g, key, k) <= 0.06 * float(np.abs(ref).max())
        # the term is there: the code and T get nothing from any other path of a normal-only loss
        assert np.abs(a['g_latent']).max() > 50 * float(g[key + '.g_latent_floor']) and np.abs(a['g_T']).max() > 50 * float(g[key + '.g_T_floor'])


def test_closed_form_matches_the_definition(restated):
    """(b) against (a) in float64: the closed form is exact wherever no ReLU sits on its kink (1e-9 of each gradient's size)."""
    g, out = restated
    for key in [k for k in out if k.endswith('_raw')]:
        a, b = out[key]
        for k in KEYS + ('g_R_product',):
            err, scale = float(np.abs(a[k] - b[k]).max()), float(np.abs(a[k]).max())
            print('%s %s: (b) - (a) %.3e of %.3e' % (key, k, err, scale))
            assert err <= 1e-9 * scale, (key, k, err, scale)


def test_unit_normals_have_no_decoder_path_term(restated):
    """The four *_unit cases: the decoder-path term of the definition is below the golden's recorded floor (scale invariance), the closed
    form returns exact zeros."""
    g, out = restated
    unit = [k for k in out if k.endswith('_unit')]
    assert len(unit) == 4
    for key in unit:
        a, b = out[key]
        for k in KEYS:
            print('%s %s: decoder-path term %.3e  floor %.3e' % (key, k, float(np.abs(a[k]).max()), float(g['%s.%s_floor' % (key, k)])))
            assert np.abs(a[k]).max() <= float(g['%s.%s_floor' % (key, k)]), (key, k)
            assert not b[k].any()
        # (what the reference returned for g_R is then the product share alone: float64 against its float32 sums, 1e-4 of the gradient's size)
        assert np.abs(a['g_R_product'] - g[key + '.g_R']).max() <= 1e-4 * np.abs(g[key + '.g_R']).max()


# ---- host side of the C ABI
def test_abi_declared_exported_and_bound():
    from distr import binding
    hdr = open(os.path.join(ROOT, 'include', 'distr_normal_grad.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    assert set(re.findall(r'\b(distr_[a-z0-9_]+)\s*\(', hdr)) == set(binding.NORMAL_GRAD_EXPORTS)
    top = open(os.path.join(ROOT, 'include', 'distr.h')).read()
    assert '#include "distr_normal_grad.h"' in top and 'DISTR_ABI_VERSION 6u' in top and binding.ABI_VERSION == 6
    assert 'distr_normal_grad.h' in binding.HEADERS and 'distr_normal_grad.hpp' in binding.SOURCES
    binding.build_library()
    L = binding.lib()
    for name in binding.NORMAL_GRAD_EXPORTS:
        assert hasattr(L, name), name
    nb = C.c_size_t()
    cfg = binding.make_cfg((8, 8), np.array([[8., 0, 4], [0, 8., 4], [0, 0, 1]]), march_step=8, buffer_size=2, normalize_normal=False)
    assert L.distr_render_normal_grad_workspace_bytes(None, C.byref(cfg), 1, C.byref(nb)) == -1          # no context: refused, not crashed
    assert L.distr_render_normal_grad_backward_batch(None, C.byref(cfg), 1, None, None, 0, None, None, None, None, None, 0, None) == -1


@pytest.fixture()
def host_ctx():
    """A context created without a device still answers the host-side questions (as in test_depth_samples_host.py)."""
    from distr import binding
    binding.build_library()
    L = binding.lib()
    h = C.c_void_p()
    L.distr_create_abi(C.byref(h), 0, binding.ABI_VERSION)
    yield L, h
    L.distr_destroy(h)


def _cfg(H=40, W=48, **kw):
    from distr import binding
    K = np.array([[48., 0, W / 2.], [0, 40., H / 2.], [0, 0, 1]])
    kw.setdefault('normalize_normal', False)
    return binding.make_cfg((H, W), K, march_step=20, buffer_size=3, marcher='recursive', **kw)


def _expected_bytes(P, nviews):
    """The layout of distr_api.hip (ng_ws, carve_list): every array on a 256-byte boundary, 256 bytes of slack for the base, per carve."""
    a = lambda n: (n + 255) // 256 * 256
    nblk = (P + 2047) // 2048                       # blocks of 2048 pixels: count / compact / camera sums
    NP = nviews * P
    tiles = nviews * ((P + 63) // 64)               # 64-point tiles of the segmented list at its capacity
    mlp = a(nviews * 1024 * 4) + a(3 * 64 * 4) + a(tiles * 1040 * 4) + 256
    return 2 * a(nviews * nblk * 4) + a(64 * 4) + a(NP * 4) + a(nviews * 1024 * 8) + a(NP * 12) + a(NP * 4) + a(NP * 12) + a(nviews * nblk * 48) + a(mlp) + 256


@pytest.mark.parametrize('H,W,nviews', [(40, 48, 1), (64, 64, 4), (137, 137, 1), (1, 1, 64), (45, 45, 3)])
def test_workspace_size_arithmetic(host_ctx, H, W, nviews):
    L, h = host_ctx
    nb = C.c_size_t()
    cfg = _cfg(H, W)
    assert L.distr_render_normal_grad_workspace_bytes(h, C.byref(cfg), nviews, C.byref(nb)) == 0, L.distr_last_error(h)
    assert nb.value == _expected_bytes(H * W, nviews)
    unit = _cfg(H, W, normalize_normal=True)        # (zeros without decoder work, the same size)
    nu = C.c_size_t()
    assert L.distr_render_normal_grad_workspace_bytes(h, C.byref(unit), nviews, C.byref(nu)) == 0 and nu.value == nb.value


def test_refusals(host_ctx):
    """Row bands, the split arithmetics, a forward without save_for_backward, depth2normal, want_normal = 0, nviews, struct size: refused
    by the size function and by the call alike, before any pointer is looked at."""
    L, h = host_ctx
    nb = C.c_size_t()
    size = lambda c, nv=1: L.distr_render_normal_grad_workspace_bytes(h, C.byref(c), nv, C.byref(nb))
    call = lambda c, nv=1: L.distr_render_normal_grad_backward_batch(h, C.byref(c), nv, None, None, 0, None, None, None, None, None, 0, None)
    INVALID, UNSUPPORTED, NO_DECODER = -1, -2, -5
    assert size(_cfg()) == 0
    assert call(_cfg()) == NO_DECODER                # a good cfg gets as far as the missing decoder
    band = _cfg()
    band.row0, band.rows = 8, 16
    arith = _cfg(arith='bf16x6')
    nosave = _cfg()
    nosave.save_for_backward = 0
    d2n = _cfg(use_depth2normal=True)
    nonormal = _cfg(want_normal=False)
    for c, code, word in ((band, UNSUPPORTED, b'row band'), (arith, UNSUPPORTED, b'arith'), (nosave, INVALID, b'save_for_backward'),
                          (d2n, INVALID, b'depth2normal'), (nonormal, INVALID, b'want_normal')):
        for fn in (size, call):
            assert fn(c) == code, (word, fn(c))
            assert word in L.distr_last_error(h), (word, L.distr_last_error(h))
    for fn in (size, call):
        assert fn(_cfg(), 0) == INVALID and fn(_cfg(), 65) == INVALID and b'nviews' in L.distr_last_error(h)
    short = _cfg()
    short.struct_size -= 4
    assert size(short) == INVALID and b'struct_size' in L.distr_last_error(h)
    assert L.distr_render_normal_grad_workspace_bytes(h, C.byref(_cfg()), 1, None) == INVALID


def test_python_option_plumbing():
    """The keyword sits behind the reference's arguments; where the term is zero or absent the option does nothing; bands raise."""
    import inspect
    from core.sdfrenderer.renderer import SDFRenderer
    from distr import functions
    params = list(inspect.signature(SDFRenderer.__init__).parameters)
    assert params[-1] == 'normal_decoder_grad' and inspect.signature(SDFRenderer.__init__).parameters['normal_decoder_grad'].default is False
    sig = inspect.signature(functions.render_batch_call)
    assert list(sig.parameters)[-1] == 'normal_decoder_grad' and sig.parameters['normal_decoder_grad'].default is False
    assert functions.normal_grad_applies(_cfg())
    assert not functions.normal_grad_applies(_cfg(normalize_normal=True))
    assert not functions.normal_grad_applies(_cfg(use_depth2normal=True))
    assert not functions.normal_grad_applies(_cfg(want_normal=False))
    band = _cfg()
    band.row0, band.rows = 8, 16
    with pytest.raises(NotImplementedError):
        functions.render_batch_call(None, band, None, None, None, normal_decoder_grad=True)
    with pytest.raises(NotImplementedError):
        functions.render_batch_call(None, _cfg(arith='bf16x6'), None, None, None, normal_decoder_grad=True)
