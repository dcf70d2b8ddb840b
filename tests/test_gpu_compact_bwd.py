"""The compacted 64-sample backward tile (k_bwd<BWD_SAVED, 2, 0, false, true>, csrc/distr_mlp.hpp "compacted 64-sample backward tile"): every
transposed layer of the dX chain walks only the hidden units that are live for the tile. A skipped link is fma(w, +0, acc) on an accumulator
that started at +0, so g_latent, g_R and g_T must be BYTE-identical to the dense backward (DISTR_DENSE_COMPACT=0 in a second context).

The size trap: bwd_range sends a list of fewer than 16 384 samples with a remainder <= 8 192 entirely to 32-sample tiles, so every test
asserts from the oracle's sample count that its list reaches the 64-sample kernel."""
import os

import numpy as np
import pytest

import helpers

pytestmark = pytest.mark.gpu

KNOB = 'DISTR_DENSE_COMPACT'
KW = dict(march_step=30, buffer_size=3, marcher='pyramid_recursive', use_depth2normal=True, ratio=1.5)
GRADS = ('g_latent', 'g_R', 'g_T')
OUTS = ('zdepth', 'mask', 'min_sdf', 'depth', 'normal')


def _engine(Ws, bs, value):
    """A context of its own with the knob set (the knobs are read at distr_create)."""
    from distr import functions
    old = os.environ.get(KNOB)
    os.environ[KNOB] = value
    try:
        return functions.engine_from_weights(Ws, bs, 0)
    finally:
        if old is None:
            del os.environ[KNOB]
        else:
            os.environ[KNOB] = old


def _reaches_64_sample_tiles(n):
    """bwd_range (csrc/distr_kernels.hpp): whole rounds of 16 384 go to 64-sample tiles, and so does everything when the remainder is
    above 8 192."""
    return n >= 16384 or (n % 16384) > 8192


def _camera(size, view):
    from distr import fixture
    return (fixture.make_intrinsic(size, size),) + tuple(helpers.bench_camera(view))


def _same(a, b, keys):
    return [k for k in keys if np.asarray(a[k]).tobytes() != np.asarray(b[k]).tobytes()]


@pytest.fixture(scope='module')
def engines(fixture_decoder):
    Ws, bs, _ = fixture_decoder
    return _engine(Ws, bs, '1'), _engine(Ws, bs, '0')


_oracle_cache = {}


def _oracle(key, O, orc, size, view, latent):
    """One CPU-oracle render per (decoder, size, view), shared by the tests and left unchanged."""
    if key not in _oracle_cache:
        K, R, T = _camera(size, view)
        _oracle_cache[key] = helpers.oracle_render(O, orc, size, size, K, R, T, latent, **KW)
    return _oracle_cache[key]


def _check_against_dense_and_oracle(on, off, ref, size, view, latent):
    K, R, T = _camera(size, view)
    n = int(ref['num_samples'])
    assert _reaches_64_sample_tiles(n), 'a list of %d samples never reaches the 64-sample kernel' % n
    a = helpers.hip_render(on, size, size, K, R, T, latent, **KW)
    b = helpers.hip_render(off, size, size, K, R, T, latent, **KW)
    assert _same(a, b, OUTS + GRADS) == []
    res = helpers.compare(a, ref, size, size, tol_depth=1e-6, tol_grad=2e-4, normal_p99=1e-5, max_flip_frac=0.0)
    print(size, view, 'samples', n, res)
    return a


@pytest.mark.parametrize('size,view', [(96, 3), (128, 0)], ids=['96_view3', '128_view0'])
def test_knob_on_equals_knob_off_f1(engines, cpu_oracle, orc, fixture_decoder, size, view):
    """96 x 96, view 3: 14 642 samples, all on 64-sample tiles, the last one partial. 128 x 128, view 0: 24 444 samples, one round of 256
    64-sample tiles and a remainder on 32-sample tiles -- both kernels write partial rows of one backward."""
    latent = fixture_decoder[2]
    ref = _oracle(('f1', size, view), cpu_oracle, orc, size, view, latent)
    if size == 128:
        n = int(ref['num_samples'])
        assert n >= 16384 and 0 < n % 16384 <= 8192, 'the case no longer runs both tile sizes (%d samples)' % n
    _check_against_dense_and_oracle(engines[0], engines[1], ref, size, view, latent)


def test_knob_on_equals_knob_off_f2(orc):
    """The non-convex fixture (torus pierced by a plate), 96 x 96."""
    from distr import fixture
    Ws, bs, latent = fixture.load_fixture_f2()
    ref = _oracle(('f2', 96, 3), orc.Oracle(Ws, bs), orc, 96, 3, latent)
    _check_against_dense_and_oracle(_engine(Ws, bs, '1'), _engine(Ws, bs, '0'), ref, 96, 3, latent)


@pytest.mark.parametrize('bias', [-1.0e3, 1.0e3], ids=['all_dead', 'all_live'])
@pytest.mark.parametrize('layer', [5, 3])
def test_edges_of_the_live_count(fixture_decoder, orc, layer, bias):
    """One hidden layer with every unit dead (bias -1e3: no live row, only the 32 zero rows are walked) or every unit live (bias +1e3: the
    list is the whole layer, the trip count at its clamp; lin3: 253 rows + padding)."""
    Ws, bs, latent = fixture_decoder
    bs2 = [b.copy() for b in bs]
    bs2[layer] = np.full_like(bs2[layer], bias)
    size, view = 96, 3
    K, R, T = _camera(size, view)
    ref = helpers.oracle_render(orc.Oracle(Ws, bs2), orc, size, size, K, R, T, latent, **KW)
    n = int(ref['num_samples'])
    assert _reaches_64_sample_tiles(n), 'a list of %d samples never reaches the 64-sample kernel' % n
    a, b = (helpers.hip_render(_engine(Ws, bs2, v), size, size, K, R, T, latent, **KW) for v in ('1', '0'))
    assert _same(a, b, OUTS + GRADS) == []
    assert all(np.isfinite(a[k]).all() for k in GRADS)


def test_batch_of_two_views(engines, cpu_oracle, orc, fixture_decoder):
    """Views 0 and 3 in one launch sequence, a code row per view: each view keeps its own tile decomposition, so its gradients equal the
    dense backward's and those of the view rendered alone."""
    import torch
    from distr import binding, functions
    latent = fixture_decoder[2]
    size, views = 96, (0, 3)
    for v in views:
        n = int(_oracle(('f1', size, v), cpu_oracle, orc, size, v, latent)['num_samples'])
        assert _reaches_64_sample_tiles(n), 'view %d: a list of %d samples never reaches the 64-sample kernel' % (v, n)
    cams = [_camera(size, v) for v in views]
    cfg = binding.make_cfg((size, size), cams[0][0], **KW)

    def batch(eng):
        dev = eng.device
        lat = torch.from_numpy(np.repeat(np.asarray(latent, np.float32).reshape(1, -1), len(views), axis=0)).to(dev).requires_grad_(True)
        Rs = torch.stack([torch.from_numpy(np.asarray(c[1], np.float32)) for c in cams]).to(dev).requires_grad_(True)
        Ts = torch.stack([torch.from_numpy(np.asarray(c[2], np.float32)) for c in cams]).to(dev).requires_grad_(True)
        outs = functions.render_batch_call(eng, cfg, lat, Rs, Ts)
        wd, wq, wn = (torch.from_numpy(x).to(dev) for x in helpers.loss_weights(size, size, 5))
        L = 0
        for v in range(len(views)):
            mb = outs[1][v].reshape(size, size).bool()
            L = L + (outs[3][v].reshape(size, size) * wd)[mb].sum() + (outs[2][v].reshape(size, size) * wq).sum() + (outs[4][v].reshape(size, size, 3) * wn).sum()
        L.backward()
        torch.cuda.synchronize()
        return dict(g_latent=lat.grad.cpu().numpy(), g_R=Rs.grad.cpu().numpy(), g_T=Ts.grad.cpu().numpy())

    on, off = batch(engines[0]), batch(engines[1])
    assert _same(on, off, GRADS) == []
    for i, (K, R, T) in enumerate(cams):
        alone = helpers.hip_render(engines[0], size, size, K, R, T, latent, **KW)
        for k in GRADS:
            assert on[k][i].tobytes() == np.asarray(alone[k]).reshape(on[k][i].shape).tobytes(), (views[i], k)
