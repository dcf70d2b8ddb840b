"""The compacted 32-ray tile (DISTR_COMPACT32 on top of DISTR_DENSE_COMPACT; csrc/distr_mlp.hpp: SmemC32, the RB = 1 forms of
compact_publish / compact_store, dense_asm_compact_n*_r1_bias): the 32-ray role of the step kernel walks only the hidden units that are > 0
for at least one of the tile's 32 rays. Point lists of 32-point tiles through distr_debug_mlp_layer32; every activation bit for bit against
the CPU oracle and against the dense 32-ray loop (DISTR_COMPACT32=0) in a second context. Every constructed decoder's live set is asserted
on the oracle before a GPU result is read."""
import numpy as np
import pytest

from test_gpu_compact import _engine, _random_points, _row_points, _subset, _with_live_units

pytestmark = pytest.mark.gpu

KNOB = 'DISTR_COMPACT32'
TILE = 32


def _pair(Ws, bs):
    """(compacted, dense) 32-ray tile: two contexts that differ in the knob only."""
    return _engine(Ws, bs, '1', {KNOB: '1'}), _engine(Ws, bs, '1', {KNOB: '0'})


def _layers32(eng, latent, pts, layers):
    import torch
    from distr import functions
    return [functions.debug_mlp_layer32(eng, torch.from_numpy(latent), torch.from_numpy(pts), l).cpu().numpy() for l in layers]


def _check_layers32(on, off, oracle, latent, pts, layers=range(8)):
    layers = list(layers)
    a, b = _layers32(on, latent, pts, layers), _layers32(off, latent, pts, layers)
    for l, x, y in zip(layers, a, b):
        width = 256 if l == 3 else 512      # (lin3 has 256 rows: what lies behind them in X is not an activation of lin3)
        ref = oracle.layer_activations(latent, pts, l)
        assert x.shape == ref.shape
        assert x[:, :width].tobytes() == ref[:, :width].tobytes(), 'layer %d differs from the oracle (max %g)' % (l, np.abs(x[:, :width] - ref[:, :width]).max())
        assert x[:, :width].tobytes() == y[:, :width].tobytes(), 'layer %d differs from the dense 32-ray loop' % l
    return a


@pytest.fixture(scope='module')
def engines(fixture_decoder):
    Ws, bs, _ = fixture_decoder
    return _pair(Ws, bs)


# ---------------------------------------------------------------------------------------- list lengths
@pytest.mark.parametrize('points', ['rows', 'cube'])
@pytest.mark.parametrize('n', [1, 31, 32, 33, 64, 65])
def test_list_lengths(engines, cpu_oracle, fixture_decoder, n, points):
    """One ray, a tile short of one ray, exactly one tile, one ray more, two tiles, two tiles and a ray: all eight layers. Coherent points
    (rows: about half of a layer's units dead per tile) and random ones (nearly every unit live)."""
    latent = fixture_decoder[2]
    pts = _row_points(n) if points == 'rows' else _random_points(n)
    acts = _check_layers32(engines[0], engines[1], cpu_oracle, latent, pts)
    if points == 'rows' and n >= TILE:
        live = [float((a[:TILE, :253 if l == 3 else 512] > 0).any(axis=0).mean()) for l, a in enumerate(acts[:7])]
        print('live fraction of the first tile per layer:', ' '.join('%.3f' % v for v in live))
        assert 0.2 < np.mean(live) < 0.9, live      # the tile really is compacted, and not to nothing


# ---------------------------------------------------------------------------------------- one live ray
# lin0 of our own: a row of W0 is zero except (for the chosen units) a 1 in the x column, so a unit's value is x + b. The x of a tile's rays
# are the 32 distinct values XS; with b between the two largest of them only the ray that holds the largest is > 0.
XS = (np.arange(TILE, dtype=np.float32) - 20.0) / 100.0          # -0.20 .. 0.11, steps of 0.01
BIAS_ONE = -np.float32(0.105)                                    # 0.11 + b > 0 > 0.10 + b

# (wave w owns units 128 w .. 128 w + 127, four blocks of 32; a lane's half-wave h holds the row groups 8 q + 4 h of a block)
ONE_RAY_UNITS = {'each_wave': [3, 128 + 41, 256 + 64, 384 + 127],
                 'halfwave_pair': [256 + 32 + 9, 256 + 32 + 13],               # rows 9 (h = 0) and 13 (h = 1) of block 1 of wave 2
                 'pairs_first_and_last_block': [0, 4, 507, 511]}


def _one_ray_points(rays):
    """32 points per entry of `rays`: tile t holds XS as its x coordinates, the largest one on ray rays[t]; y and z are small and distinct."""
    tiles = []
    for t, ray in enumerate(rays):
        x = np.empty(TILE, np.float32)
        x[np.delete(np.arange(TILE), ray)] = XS[np.random.RandomState(10 + t).permutation(TILE - 1)]
        x[ray] = XS[TILE - 1]
        rs = np.random.RandomState(20 + t)
        tiles.append(np.stack([x, (rs.rand(TILE) * 0.2 - 0.1).astype(np.float32), (rs.rand(TILE) * 0.2 - 0.1).astype(np.float32)], axis=1))
    return np.ascontiguousarray(np.concatenate(tiles), dtype=np.float32)


def _one_ray_decoder(fixture_decoder, units):
    Ws, bs, _ = fixture_decoder
    W0, b0 = np.zeros_like(Ws[0]), np.full_like(bs[0], -1.0)
    W0[units, Ws[0].shape[1] - 3] = 1.0          # input = [latent | x y z]
    b0[units] = BIAS_ONE
    return [W0] + [w.copy() for w in Ws[1:]], [b0] + [b.copy() for b in bs[1:]]


@pytest.mark.parametrize('ray', [0, 15, 16, 31])
@pytest.mark.parametrize('name', sorted(ONE_RAY_UNITS))
def test_unit_live_for_one_ray(fixture_decoder, name, ray):
    """The OR over the tile's 32 rays must see a single lane: rays 0 / 31 are the ends of a half-wave's lanes, 15 / 16 the middle the
    butterfly's last exchange crosses. Two tiles; the second has its live ray at 31 - ray."""
    from oracle import oracle as orc
    latent = fixture_decoder[2]
    units = ONE_RAY_UNITS[name]
    rays = [ray, TILE - 1 - ray]
    Ws, bs = _one_ray_decoder(fixture_decoder, units)
    pts = _one_ray_points(rays)
    oracle = orc.Oracle(Ws, bs)
    want = np.zeros((TILE * len(rays), 512), bool)
    for t, r in enumerate(rays):
        want[TILE * t + r, units] = True
    assert ((oracle.layer_activations(latent, pts, 0) > 0) == want).all(), 'the case does not have the live set it was built for'
    on, off = _pair(Ws, bs)
    _check_layers32(on, off, oracle, latent, pts, layers=(0, 1, 7))


# ---------------------------------------------------------------------------------------- live counts
COUNTS = (0, 1, 15, 16, 17, 31, 32, 33, 511, 512)
COUNTS_LIN3 = (0, 1, 13, 29, 253)             # (+ the three xyz rows: 13 + 3 and 29 + 3 are the granule edges)


def _check_live_set(fixture_decoder, layer, live, pts):
    """F1 with exactly `live` > 0 on `layer` (for every ray): the oracle has that live set, and the engines agree with it bit for bit."""
    from oracle import oracle as orc
    latent = fixture_decoder[2]
    live = np.asarray(live, dtype=np.int64)
    Ws, bs = _with_live_units(fixture_decoder, layer, live)
    oracle = orc.Oracle(Ws, bs)
    width = 253 if layer == 3 else 512
    want = np.zeros(width, bool)
    want[live] = True
    assert ((oracle.layer_activations(latent, pts, layer)[:, :width] > 0) == want[None, :]).all(), 'the case does not have the live set it was built for'
    on, off = _pair(Ws, bs)
    _check_layers32(on, off, oracle, latent, pts, layers=sorted({layer, min(layer + 1, 7), 7}))


@pytest.mark.parametrize('count', COUNTS)
@pytest.mark.parametrize('layer', [0, 4, 5, 6])
def test_live_count_edges(fixture_decoder, layer, count):
    """Padding only, one unit, the counts around the padding granule (16) and the minimum trip count (32), all but one and all units, behind
    lin0 (the write-back behind the C++ k-loop) and lin4..lin6. Two tiles and a partial one."""
    _check_live_set(fixture_decoder, layer, _subset(count, 512, 1000 * layer + count), _row_points(2 * TILE + 7))


@pytest.mark.parametrize('count', COUNTS_LIN3)
def test_live_count_edges_lin3(fixture_decoder, count):
    """lin3 -> lin4: 253 rows in two blocks per wave, the three xyz rows (32 wide) appended behind the live ones; with no live row lin4 sees
    xyz only."""
    _check_live_set(fixture_decoder, 3, _subset(count, 253, 300 + count), _row_points(2 * TILE + 7))


# ---------------------------------------------------------------------------------------- live sets confined to one part of the layer
CONFINED = [('lin2_wave0_full', 2, np.arange(0, 128)), ('lin2_wave2_sparse', 2, 256 + _subset(40, 128, 7)), ('lin2_last_block', 2, np.arange(480, 512)),
            ('lin5_wave1_sparse', 5, 128 + _subset(23, 128, 8)), ('lin5_last_block_sparse', 5, 480 + _subset(9, 32, 9)),
            ('lin0_wave1_full', 0, np.arange(128, 256)), ('lin0_last_block', 0, np.arange(480, 512)),
            # lin3: 253 rows, two blocks per wave (wave w owns rows 64 w .. 64 w + 63)
            ('lin3_wave1_full', 3, np.arange(64, 128)), ('lin3_last_block', 3, np.arange(224, 253))]


@pytest.mark.parametrize('name,layer,live', CONFINED, ids=[c[0] for c in CONFINED])
def test_live_units_confined(fixture_decoder, name, layer, live):
    """All live units in one wave (the other three publish zero words: their bases and the total come from one wave's counts alone), and all
    in the last block of the last wave (every position counts the empty words below it)."""
    _check_live_set(fixture_decoder, layer, live, _row_points(TILE + 5))


# ---------------------------------------------------------------------------------------- the knob
def test_knob_needs_the_64_ray_knob(fixture_decoder, cpu_oracle):
    """DISTR_COMPACT32=1 with DISTR_DENSE_COMPACT=0: no k-major pack, every tile dense -- the same bytes."""
    Ws, bs, latent = fixture_decoder
    pts = _row_points(TILE + 5)
    _check_layers32(_engine(Ws, bs, '0', {KNOB: '1'}), _engine(Ws, bs, '1', {KNOB: '0'}), cpu_oracle, latent, pts, layers=(0, 3, 7))


@pytest.mark.parametrize('value', ['2', '-1', 'on', ''])
def test_illegal_knob_value_is_refused(fixture_decoder, value):
    from distr import binding
    Ws, bs, _ = fixture_decoder
    with pytest.raises(binding.DistrError, match=KNOB):
        _engine(Ws, bs, '1', {KNOB: value})
