#!/usr/bin/env python
"""Live fraction of the hidden units per 64-sample backward tile, counted on the CPU oracle (no GPU needed).

The compacted backward tile (csrc/distr_mlp.hpp, "compacted 64-sample backward tile") walks, per transposed layer, only the hidden units
that are > 0 for at least one of the tile's 64 gradient samples. What it saves is therefore decided by how coherent a tile's samples are.
This tool renders a view with the oracle, takes the gradient samples of the benchmark's dense loss (RenderState.samples), re-orders them the
way k_bwd_prep<true> emits them -- 256-pixel block, then buffer row, then pixel -- cuts the list into 64-sample tiles and evaluates
Oracle.layer_activations on evenly spaced tiles.

The oracle lists a pixel's samples in buffer-row order and drops rows whose coefficient is zero, so a sample's buffer row is taken as its
rank among the pixel's listed samples (exact unless a row in the middle of a pixel's buffer has a zero coefficient). The combined pad
sample, if any, is left out.

  python profiles/tools/live_fraction_bwd.py [--fixture f1|f2] [--size 512] [--view 0] [--steps 50] [--tiles 160] [--shuffle]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (os.path.join(ROOT, 'dist-renderer_amd'), ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)


def gpu_order(pix):
    """Permutation of the oracle's sample list into k_bwd_prep<true>'s emission order."""
    rank = np.zeros(len(pix), np.int64)
    seen = {}
    for i, p in enumerate(pix.tolist()):
        rank[i] = seen.get(p, 0)
        seen[p] = rank[i] + 1
    return np.lexsort((pix, rank, pix // 256))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--fixture', default='f1', choices=['f1', 'f2'])
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--view', type=int, default=0)
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--tiles', type=int, default=160)
    ap.add_argument('--shuffle', action='store_true', help='the same samples in random order (what an incoherent list would give)')
    args = ap.parse_args(argv)
    import helpers
    from distr import fixture
    from oracle import oracle as orc
    orc.build()
    Ws, bs, latent = fixture.make_decoder_weights() if args.fixture == 'f1' else fixture.load_fixture_f2()
    O = orc.Oracle(Ws, bs)
    H = W = args.size
    K = fixture.make_intrinsic(H, W)
    R, T = helpers.bench_camera(args.view)
    cfg = orc.make_cfg(H, W, K, march_step=args.steps, buffer_size=3, marcher='pyramid_recursive', use_depth2normal=True)
    out = O.render(cfg, latent, R, T)
    wd, wq, wn = helpers.loss_weights(H, W, 5)
    m = out['mask'].reshape(H, W).astype(np.float32)
    pix, pts, _ = out['state'].samples(g_min_sdf=wq.reshape(-1), g_depth=(wd * m).reshape(-1), g_normal=wn.reshape(-1))
    keep = pix >= 0
    pix, pts = pix[keep], pts[keep]
    order = np.random.RandomState(0).permutation(len(pix)) if args.shuffle else gpu_order(pix)
    pts = pts[order]
    ntiles = len(pts) // 64
    pick = np.unique(np.linspace(0, ntiles - 1, min(args.tiles, ntiles)).astype(np.int64))
    idx = (pick[:, None] * 64 + np.arange(64)[None, :]).reshape(-1)
    live = np.zeros((8, len(pick)))
    for l in range(8):
        width = 253 if l == 3 else 512
        act = O.layer_activations(latent, pts[idx], l)[:, :width].reshape(len(pick), 64, width)
        live[l] = (act > 0).any(axis=1).mean(axis=1)
    print('%s %dx%d view %d, %d steps: %d gradient samples, %d whole 64-sample tiles, %d counted, order: %s' %
          (args.fixture, H, W, args.view, args.steps, len(pts), ntiles, len(pick), 'shuffled' if args.shuffle else 'k_bwd_prep'))
    print('layer          ' + ' '.join('%6d' % l for l in range(8)))
    print('mean over tiles' + ' '.join('%6.3f' % v for v in live.mean(axis=1)))
    print('max over tiles ' + ' '.join('%6.3f' % v for v in live.max(axis=1)))
    print('mean of layers 1..7 (the K operands of the backward chain): %.3f' % live[1:].mean())
    return 0


if __name__ == '__main__':
    sys.exit(main())
