"""The compacted 64-ray tile (DISTR_DENSE_COMPACT, csrc/distr_mlp.hpp "compacted 64-ray tile"): a layer walks only the hidden units that
are > 0 for at least one ray of the tile. Skipping a unit that is +0 for every ray removes no-op links from the k-ordered fma chains, so
every activation, output and gradient must be BIT-identical to the oracle and to the dense loop (knob 0) in a second context."""
import os

import numpy as np
import pytest

import helpers

pytestmark = pytest.mark.gpu

KNOB = 'DISTR_DENSE_COMPACT'


def _engine(Ws, bs, value, extra=None):
    """A context of its own with the knob set (the knobs are read at distr_create)."""
    from distr import functions
    env = {KNOB: value}
    env.update(extra or {})
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return functions.engine_from_weights(Ws, bs, 0)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


@pytest.fixture(scope='module')
def engines(fixture_decoder):
    Ws, bs, _ = fixture_decoder
    return _engine(Ws, bs, '1'), _engine(Ws, bs, '0')


def _row_points(n, row=256, col0=150, depth=1.6, size=512):
    """n points of consecutive pixels of one image row of the headline camera (bench view 0, 512 x 512) at one march depth: coherent
    tiles, about 0.57 of a layer's units live per tile."""
    from distr import fixture
    K = fixture.make_intrinsic(size, size)
    R, T = helpers.bench_camera(0)
    u = np.arange(col0, col0 + n, dtype=np.float64) + 0.5
    pix = np.stack([u, np.full(n, row + 0.5), np.ones(n)], axis=0)
    pc = depth * (np.linalg.inv(K) @ pix)
    pw = R.astype(np.float64).T @ (pc - T.astype(np.float64).reshape(3, 1))
    p = np.ascontiguousarray(pw.T, dtype=np.float32)
    assert (np.linalg.norm(p, axis=1) < 1.0).all()
    return p


def _random_points(n, seed=3):
    rs = np.random.RandomState(seed)
    p = (rs.rand(n, 3) * 1.8 - 0.9).astype(np.float32)
    p[:4] = 0.0
    return p


def _layers(eng, latent, pts, layers=range(8)):
    import torch
    from distr import functions
    return [functions.debug_mlp_layer(eng, torch.from_numpy(latent), torch.from_numpy(pts), l).cpu().numpy() for l in layers]


def _check_layers(on, off, oracle, latent, pts, layers=range(8)):
    layers = list(layers)
    a, b = _layers(on, latent, pts, layers), _layers(off, latent, pts, layers)
    for l, x, y in zip(layers, a, b):
        width = 256 if l == 3 else 512
        ref = oracle.layer_activations(latent, pts, l)
        assert x[:, :width].tobytes() == ref[:, :width].tobytes(), 'layer %d differs from the oracle (max %g)' % (l, np.abs(x[:, :width] - ref[:, :width]).max())
        # (lin3 has 256 rows: the rows of X behind them are whatever the earlier layers left there, not activations of lin3)
        assert x[:, :width].tobytes() == y[:, :width].tobytes(), 'layer %d differs from the dense loop' % l
    return a


N_PTS = 64 * 2 + 17      # two full tiles and a partial one


def test_layers_bitwise_coherent_tiles(engines, cpu_oracle, fixture_decoder):
    """Points along one image row: a large share of every layer's units is dead for the whole tile (the case the loop is built for)."""
    _, _, latent = fixture_decoder
    pts = _row_points(N_PTS)
    acts = _check_layers(engines[0], engines[1], cpu_oracle, latent, pts)
    live = [float((a[:64] > 0).any(axis=0).mean()) for a in acts[:7]]
    print('live fraction of the first tile per layer:', ' '.join('%.3f' % v for v in live))
    assert 0.2 < np.mean(live) < 0.9, live      # the tiles really are compacted, and not to nothing


def test_layers_bitwise_incoherent_tiles(engines, cpu_oracle, fixture_decoder):
    """Random points of the cube: nearly every unit is live for some ray (lists of about 512 entries)."""
    _, _, latent = fixture_decoder
    _check_layers(engines[0], engines[1], cpu_oracle, latent, _random_points(N_PTS))


def test_all_rays_at_the_same_point(engines, cpu_oracle, fixture_decoder):
    _, _, latent = fixture_decoder
    pts = np.repeat(np.array([[0.11, -0.07, 0.23]], np.float32), 64 + 17, axis=0)
    _check_layers(engines[0], engines[1], cpu_oracle, latent, pts)


def _with_live_units(fixture_decoder, layer, live):
    """F1 with the bias of `layer` overwritten: exactly the units in `live` are > 0 (for every ray), all others far below 0."""
    Ws, bs, _ = fixture_decoder
    bs2 = [b.copy() for b in bs]
    b = np.full_like(bs2[layer], -1.0e4)
    b[np.asarray(live, dtype=np.int64)] = 1.0e2
    bs2[layer] = b
    return Ws, bs2


def _subset(n, width, seed):
    return np.sort(np.random.RandomState(seed).choice(width, n, replace=False))


EDGE_512 = [('none', []), ('one_0', [0]), ('one_127', [127]), ('one_128', [128]), ('one_511', [511])] + \
           [('n%d' % n, _subset(n, 512, n)) for n in (15, 16, 17, 31, 32, 33)] + [('all', np.arange(512))]
EDGE_253 = [('none', []), ('one_0', [0]), ('one_63', [63]), ('one_64', [64]), ('one_252', [252])] + \
           [('n%d' % n, _subset(n, 253, 100 + n)) for n in (12, 13, 14, 28, 29, 30)] + [('all', np.arange(253))]


def _check_edge(fixture_decoder, layer, live):
    from oracle import oracle as orc
    latent = fixture_decoder[2]
    Ws, bs = _with_live_units(fixture_decoder, layer, live)
    on, off = _engine(Ws, bs, '1'), _engine(Ws, bs, '0')
    pts = _row_points(64 + 17)
    acts = _check_layers(on, off, orc.Oracle(Ws, bs), latent, pts, layers=(layer, layer + 1, 7))
    width = 253 if layer == 3 else 512
    got = np.flatnonzero((acts[0][:, :width] > 0).any(axis=0))
    assert got.tolist() == list(np.asarray(live, dtype=np.int64).tolist()), 'the case does not have the live units it was built for'


@pytest.mark.parametrize('name,live', EDGE_512, ids=[c[0] for c in EDGE_512])
def test_edge_counts_lin1_to_lin2(fixture_decoder, name, live):
    """Live counts at the edges of the list: padding only, one unit at the first / last feature and at a wave boundary, counts around the
    padding granule (16) and the minimum trip count (32), and the full list."""
    _check_edge(fixture_decoder, 1, live)


@pytest.mark.parametrize('name,live', EDGE_253, ids=[c[0] for c in EDGE_253])
def test_edge_counts_lin3_to_lin4(fixture_decoder, name, live):
    """The same on lin3 -> lin4: 253 rows compacted, the three xyz rows appended (so 13 + 3, 29 + 3 ... are the granule edges); with no
    live row lin4 sees xyz only."""
    _check_edge(fixture_decoder, 3, live)


RENDERS = [dict(H=64, march_step=20, buffer_size=3, marcher='pyramid_recursive', use_depth2normal=True, cam=(30, 20, 1.6, 10)),
           dict(H=96, march_step=30, buffer_size=3, marcher='recursive', use_depth2normal=False, cam=(35.0, 25.0, 1.6, 10.0))]


@pytest.mark.parametrize('save_masks', ['1', '0'])
@pytest.mark.parametrize('case', range(len(RENDERS)))
def test_renders_identical_knob_on_and_off(fixture_decoder, case, save_masks):
    """Outputs and gradients of a render, saved masks on and off: the mask blocks keep their layout under the k-major pack's row order."""
    from distr import fixture
    Ws, bs, latent = fixture_decoder
    kw = dict(RENDERS[case])
    H = W = kw.pop('H')
    R, T = fixture.make_camera(*kw.pop('cam'))
    K = fixture.make_intrinsic(H, W)
    outs = [helpers.hip_render(_engine(Ws, bs, v, {'DISTR_SAVE_MASKS': save_masks}), H, W, K, R, T, latent, **kw) for v in ('1', '0')]
    assert outs[0]['mask'].sum() > 100
    for k in ('zdepth', 'mask', 'min_sdf', 'depth', 'normal', 'g_latent', 'g_R', 'g_T'):
        assert outs[0][k].tobytes() == outs[1][k].tobytes(), k


def test_decode_sdf_identical_knob_on_and_off(engines, cpu_oracle, fixture_decoder):
    import torch
    from distr import functions
    _, _, latent = fixture_decoder
    for pts in (_random_points(4096 + 37), _row_points(300, col0=100)):
        a, b = (functions.mlp_eval(e, torch.from_numpy(latent), torch.from_numpy(pts)).cpu().numpy() for e in engines)
        assert a.tobytes() == b.tobytes()
        assert np.abs(a.reshape(-1) - cpu_oracle.decode_sdf(latent, pts)).max() <= 1e-7


@pytest.mark.parametrize('value', ['2', '-1', 'on', ''])
def test_illegal_knob_value_is_refused(fixture_decoder, value):
    from distr import binding
    Ws, bs, _ = fixture_decoder
    with pytest.raises(binding.DistrError, match=KNOB):
        _engine(Ws, bs, value)
