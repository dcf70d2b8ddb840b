"""tests/bwd_list_restatement.py on the CPU: the tile plan that aims tests/test_gpu_bwd_list.py is a partition of the list for every
count, fits what render_backward_impl allocates and launches, and the float64 code gradient equals train_restatement.gradients."""
import numpy as np
import pytest

import bwd_list_restatement as bl
import train_restatement as tr

COUNTS = range(0, 40001)


@pytest.mark.parametrize('split', [True, False])
def test_tile_plan_partitions_every_count(split):
    """Every list position lies in exactly one tile, the partial rows are 0 .. ntiles - 1 without gaps, ntiles fits the partial rows the
    host allocates and every launch_bwd grid covers its kernel's tiles -- for the smallest workspace a list of that length can have
    (smax = count: both sizes grow with smax)."""
    for n in COUNTS:
        p = bl.tile_plan(n, split)
        lo, hi, row, size = p['lo'], p['hi'], p['row'], p['size']
        assert len(row) == p['ntiles'], n
        if n == 0:
            assert p['ntiles'] == 0 and p['nchunks'] == 0
            continue
        o = np.argsort(lo, kind='stable')
        assert lo[o][0] == 0 and hi[o][-1] == n and np.array_equal(lo[o][1:], hi[o][:-1]), n      # a partition of [0, n) ...
        assert (hi > lo).all() and (hi - lo <= size).all(), n                                       # ... into tiles that hold a sample
        assert ((hi - lo == size) | (hi == n) | (hi == p['full'])).all(), n                         # short only at the end of a range
        assert np.array_equal(np.sort(row), np.arange(p['ntiles'])), n
        assert np.array_equal(row[o], np.arange(p['ntiles'])), n                                    # rows ascend with the list
        assert p['ntiles'] <= bl.prows(n), n
        assert p['nchunks'] * bl.BWD_CHUNK >= p['ntiles'] > (p['nchunks'] - 1) * bl.BWD_CHUNK, n
        assert p['nchunks'] <= (bl.prows(n) + bl.BWD_CHUNK - 1) // bl.BWD_CHUNK, n                  # nchunks_max of k_bwd_final
        grids = bl.launch_grids(n, split)
        assert set(grids) == set(p['per_kernel']), n
        for ts, tiles in p['per_kernel'].items():
            assert tiles <= grids[ts], (n, ts, tiles, grids)
        if split:
            rem = n % bl.ROUND
            assert p['full'] == (n if rem > bl.REM_MAX else n - rem), n
            assert (size[lo < p['full']] == 64).all() and (size[lo >= p['full']] == 32).all(), n
        else:
            assert p['full'] == n and (size == 64).all(), n


def test_plan_at_the_edges_the_gpu_module_runs():
    """The counts the GPU module runs sit where they are meant to: 32-sample tiles up to 8 192, 64-sample tiles above, the hand-over behind a
    whole round, and the 64th partial row."""
    assert bl.tile_plan(8192, True)['per_kernel'] == {64: 0, 32: 256}
    assert bl.tile_plan(8193, True)['per_kernel'] == {64: 129, 32: 0}
    assert bl.tile_plan(16384, True)['per_kernel'] == {64: 256, 32: 0}
    assert bl.tile_plan(16385, True)['per_kernel'] == {64: 256, 32: 1}
    assert bl.tile_plan(16417, True)['per_kernel'] == {64: 256, 32: 2}
    assert bl.tile_plan(24576, True)['per_kernel'] == {64: 256, 32: 256}
    assert bl.tile_plan(24577, True)['per_kernel'] == {64: 385, 32: 0}
    assert bl.tile_plan(16385, False)['per_kernel'] == {64: 257}
    assert bl.edge_positions(0, True) == []
    assert bl.edge_positions(1, True) == [0]
    assert bl.edge_positions(2049, True) == [0, 2048]                                   # row 64 is the last tile: one sample
    assert bl.edge_positions(4097, True) == [0, 2048, 4096]                             # rows 64 and 128
    assert bl.edge_positions(4097, False) == [0, 4096]                                  # row 64 of 64-sample tiles
    assert bl.edge_positions(16417, True) == [0, 4096, 8192, 12288, 16383, 16384, 16416]
    assert bl.edge_positions(24577, True) == [0, 4096, 8192, 12288, 16384, 20480, 24576]
    per, own = bl.scan_plan(273)
    assert per == 2 and own[-1] == (136, 272, 273) and len(own) == 137                  # thread 136 owns block 272 alone
    assert bl.scan_plan(1024)[0] == 4 and bl.scan_plan(100) == (1, [(t, t, t + 1) for t in range(100)])


def test_unit_code_gradients_match_train_restatement(fixture_decoder):
    """64 samples: the rows equal train_restatement.gradients(...)[4] with unit weights, on float64's own ReLU pattern and on a given
    one (a random pattern: nothing here depends on which), and the chunked walk changes nothing."""
    import torch
    Ws, bs, latent = fixture_decoder
    rs = np.random.RandomState(3)
    pts = (rs.rand(64, 3) * 1.2 - 0.6).astype(np.float32)
    codes = np.repeat(latent, 64, 0)
    ones = np.ones(64, np.float32)
    gates = [rs.rand(64, Ws[l].shape[0]) > 0.5 for l in range(8)]
    for g in (None, gates):
        ref = tr.gradients(Ws, bs, codes, pts, [1] * 64, ones, gates=None if g is None else [torch.from_numpy(m) for m in g])[4].numpy()
        assert ref.shape == (64, 256) and np.abs(ref).max() > 0
        for chunk in (2048, 24):
            got = bl.unit_code_gradients(Ws, bs, latent, pts, g, chunk=chunk)
            assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max(), (g is None, chunk)
