"""The compacting write-back of the 64-ray tile (csrc/distr_mlp.hpp: compact_publish, compact_store) at the edges a publish / store can
get wrong and tests/test_gpu_compact.py does not reach: a unit that is live for a single ray of the tile (at the edges of the half-waves
and of the two 32-ray blocks), the live-count edges on the boundaries behind lin0 and lin4..lin6, live sets confined to one wave or to
the last block of the last wave, and a tile with one real ray. Point lists only (debug_mlp_layer, distr_mlp_eval), no renders; every
activation bit for bit against the CPU oracle and against the dense loop (knob 0) in a second context."""
import numpy as np
import pytest

from test_gpu_compact import _check_layers, _engine, _random_points, _row_points, _subset, _with_live_units

pytestmark = pytest.mark.gpu


def _check_eval(on, off, latent, pts):
    import torch
    from distr import functions
    a, b = (functions.mlp_eval(e, torch.from_numpy(latent), torch.from_numpy(pts)).cpu().numpy() for e in (on, off))
    assert a.tobytes() == b.tobytes(), 'distr_mlp_eval differs from the dense loop'


# ---------------------------------------------------------------------------------------- one live ray
# lin0 of our own: a row of W0 is zero except (for the chosen units) a 1 in the x column, so a unit's value is x + b. The x of a tile's
# rays are the 64 distinct values XS; with b between the two largest of them only the ray that holds the largest is > 0.
XS = (np.arange(64, dtype=np.float32) - 50.0) / 100.0            # -0.50 .. 0.13, steps of 0.01
BIAS_ONE = -np.float32(0.125)                                    # 0.13 + b > 0 > 0.12 + b

# (wave w owns units 128 w .. 128 w + 127, four blocks of 32; a lane's half-wave h holds the row groups 8 q + 4 h of a block)
ONE_RAY_UNITS = {'each_wave': [3, 128 + 41, 256 + 64, 384 + 127],
                 'halfwave_pair': [256 + 32 + 9, 256 + 32 + 13],               # rows 9 (h = 0) and 13 (h = 1) of block 1 of wave 2
                 'pairs_first_and_last_block': [0, 4, 507, 511]}


def _one_ray_points(rays):
    """64 points per entry of `rays`: tile t holds XS as its x coordinates, the largest one on ray rays[t]; y and z are small and distinct."""
    tiles = []
    for t, ray in enumerate(rays):
        x = np.empty(64, np.float32)
        x[np.delete(np.arange(64), ray)] = XS[np.random.RandomState(10 + t).permutation(63)]
        x[ray] = XS[63]
        rs = np.random.RandomState(20 + t)
        tiles.append(np.stack([x, (rs.rand(64) * 0.2 - 0.1).astype(np.float32), (rs.rand(64) * 0.2 - 0.1).astype(np.float32)], axis=1))
    return np.ascontiguousarray(np.concatenate(tiles), dtype=np.float32)


def _one_ray_decoder(fixture_decoder, units):
    Ws, bs, _ = fixture_decoder
    W0, b0 = np.zeros_like(Ws[0]), np.full_like(bs[0], -1.0)
    W0[units, Ws[0].shape[1] - 3] = 1.0          # input = [latent | x y z]
    b0[units] = BIAS_ONE
    return [W0] + [w.copy() for w in Ws[1:]], [b0] + [b.copy() for b in bs[1:]]


@pytest.mark.parametrize('ntile', [1, 2], ids=['64pts', '128pts'])
@pytest.mark.parametrize('ray', [0, 31, 32, 63])
@pytest.mark.parametrize('name', sorted(ONE_RAY_UNITS))
def test_unit_live_for_one_ray(fixture_decoder, name, ray, ntile):
    """The OR over the tile's rays must see a single lane of a single 32-ray block: ray 0 / 31 are the ends of block 0 (and of the lanes of
    a half-wave), 32 / 63 those of block 1. The second tile of the 128-point list has its live ray at 63 - ray."""
    from oracle import oracle as orc
    latent = fixture_decoder[2]
    units = ONE_RAY_UNITS[name]
    rays = [ray, 63 - ray][:ntile]
    Ws, bs = _one_ray_decoder(fixture_decoder, units)
    pts = _one_ray_points(rays)
    oracle = orc.Oracle(Ws, bs)
    want = np.zeros((64 * ntile, 512), bool)
    for t, r in enumerate(rays):
        want[64 * t + r, units] = True
    assert ((oracle.layer_activations(latent, pts, 0) > 0) == want).all(), 'the case does not have the live set it was built for'
    on, off = _engine(Ws, bs, '1'), _engine(Ws, bs, '0')
    _check_layers(on, off, oracle, latent, pts, layers=(0, 1, 7))
    _check_eval(on, off, latent, pts)


# ---------------------------------------------------------------------------------------- live counts behind lin0, lin4, lin5, lin6
COUNTS = (0, 1, 15, 16, 17, 31, 32, 33, 511, 512)


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
    on, off = _engine(Ws, bs, '1'), _engine(Ws, bs, '0')
    _check_layers(on, off, oracle, latent, pts, layers=sorted({layer, min(layer + 1, 7), 7}))
    _check_eval(on, off, latent, pts)


@pytest.mark.parametrize('count', COUNTS)
@pytest.mark.parametrize('layer', [0, 4, 5, 6])
def test_live_count_edges(fixture_decoder, layer, count):
    """Padding only, one unit, the counts around the padding granule (16) and the minimum trip count (32), all but one and all units, on the
    boundaries the existing edge tests leave out (lin0: the write-back behind the C++ k-loop; lin4..lin6: the second half of the chain)."""
    _check_live_set(fixture_decoder, layer, _subset(count, 512, 1000 * layer + count), _row_points(128))


# ---------------------------------------------------------------------------------------- live sets confined to one part of the layer
CONFINED = [('lin2_wave0_full', 2, np.arange(0, 128)), ('lin2_wave2_sparse', 2, 256 + _subset(40, 128, 7)), ('lin2_last_block', 2, np.arange(480, 512)),
            ('lin5_wave3_full', 5, np.arange(384, 512)), ('lin5_wave1_sparse', 5, 128 + _subset(23, 128, 8)), ('lin5_last_block_sparse', 5, 480 + _subset(9, 32, 9)),
            ('lin0_wave1_full', 0, np.arange(128, 256)), ('lin0_last_block', 0, np.arange(480, 512)),
            # lin3: 253 rows, two blocks per wave (wave w owns rows 64 w .. 64 w + 63)
            ('lin3_wave1_full', 3, np.arange(64, 128)), ('lin3_last_block', 3, np.arange(224, 253))]


@pytest.mark.parametrize('name,layer,live', CONFINED, ids=[c[0] for c in CONFINED])
def test_live_units_confined(fixture_decoder, name, layer, live):
    """All live units in one wave (the other three publish zero words: their bases and the total come from one wave's counts alone), and all
    in the last block of the last wave (every position counts the empty words below it)."""
    _check_live_set(fixture_decoder, layer, live, _row_points(64))


# ---------------------------------------------------------------------------------------- a tile with one real ray
@pytest.mark.parametrize('points', ['rows', 'cube'])
def test_second_tile_holds_one_ray(fixture_decoder, cpu_oracle, points):
    """65 points: the second tile's live sets are those of its one real ray and of whatever the padding rays hold."""
    Ws, bs, latent = fixture_decoder
    pts = _row_points(65) if points == 'rows' else _random_points(65)
    on, off = _engine(Ws, bs, '1'), _engine(Ws, bs, '0')
    _check_layers(on, off, cpu_oracle, latent, pts)
    _check_eval(on, off, latent, pts)


def test_second_tile_one_ray_one_live_unit(fixture_decoder):
    """65 points, and the only live units of lin0 in the second tile are live for its one real ray."""
    from oracle import oracle as orc
    latent = fixture_decoder[2]
    units = ONE_RAY_UNITS['each_wave']
    Ws, bs = _one_ray_decoder(fixture_decoder, units)
    pts = _one_ray_points([32])
    last = pts[32:33].copy()
    pts = np.ascontiguousarray(np.concatenate([pts, last]), dtype=np.float32)
    oracle = orc.Oracle(Ws, bs)
    act = oracle.layer_activations(latent, pts, 0) > 0
    assert act[64, units].all() and act[64].sum() == len(units) and act[:64].sum() == len(units)
    on, off = _engine(Ws, bs, '1'), _engine(Ws, bs, '0')
    _check_layers(on, off, oracle, latent, pts, layers=(0, 1, 7))
    _check_eval(on, off, latent, pts)
