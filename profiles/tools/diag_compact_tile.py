"""Phase stamps of the 64-ray decoder tile on COHERENT points (not a pytest file): the points are consecutive pixels of image rows of the
headline camera at one march depth -- the tiles a render evaluates, with about 0.55 of a layer's units live per tile -- or, with --cube,
random points of the cube (nearly every unit live for some ray: what tests/gpu_diag_dense.py feeds). Prints the time of distr_mlp_eval,
the per-layer MFMA / write-back stamps of wave 0 (shader clock), the tile total, and the live fraction per layer counted on the device.
DISTR_DENSE_COMPACT=0|1 in the environment chooses the loop (read at distr_create).

    python profiles/tools/diag_compact_tile.py [--n 65536] [--reps 10] [--cube] [--tile 32 --n 8192]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (os.path.join(ROOT, 'dist-renderer_amd'), ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)
import numpy as np
import torch

FLOP = 3146752      # algorithmic FLOP per decoder evaluation (skipped products included)
PEAK = 157.3


def row_points(n, depth=1.6, size=512):
    """The 384 central pixels of as many image rows around the centre as it takes, at `depth` (the plane through the object's centre):
    all inside the unit sphere; 64 consecutive points = one tile."""
    import helpers
    from distr import fixture
    K = fixture.make_intrinsic(size, size)
    R, T = helpers.bench_camera(0)
    nrow = (n + 383) // 384
    u, v = np.meshgrid(np.arange(64, 448) + 0.5, size // 2 - nrow // 2 + np.arange(nrow) + 0.5)
    pc = depth * (np.linalg.inv(K) @ np.stack([u.ravel(), v.ravel(), np.ones(u.size)]))
    p = (R.astype(np.float64).T @ (pc - T.astype(np.float64).reshape(3, 1))).T[:n]
    return np.ascontiguousarray(p, dtype=np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=65536)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--cube', action='store_true', help='random points of the cube instead of image rows')
    ap.add_argument('--tile', type=int, default=64, choices=[64, 32], help='32: the 32-point tile of the step kernel\'s 32-ray role (DISTR_COMPACT32=0|1 chooses its loop); '
                    'use --n 8192 for one tile per compute unit, as the role runs')
    args = ap.parse_args()
    from distr import fixture, functions
    Ws, bs, latent = fixture.make_decoder_weights()
    eng = functions.engine_from_weights(Ws, bs, 0)
    if args.cube:
        pts_np = (np.random.RandomState(3).rand(args.n, 3) * 1.6 - 0.8).astype(np.float32)
    else:
        pts_np = row_points(args.n)
    pts = torch.from_numpy(pts_np).cuda()
    lat = torch.from_numpy(latent).cuda()
    for _ in range(3):
        functions.mlp_eval(eng, lat, pts)
    ts = []
    for _ in range(args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); functions.mlp_eval(eng, lat, pts); e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    med = float(np.median(ts))
    print('points: %s; DISTR_DENSE_COMPACT=%s' % ('cube' if args.cube else 'image rows', os.environ.get('DISTR_DENSE_COMPACT', '(default)')))
    print('distr_mlp_eval n=%d: median %.3f ms (min %.3f) = %.1f algorithmic TFLOP/s = %.3f of the f32-MFMA peak'
          % (args.n, med, min(ts), FLOP * args.n / med / 1e9, FLOP * args.n / med / 1e9 / PEAK))
    T = args.tile
    nst = min(args.n, 256 * 64 * 4) // T * T
    print('stamps: %d tiles of %d points; DISTR_COMPACT32=%s' % (nst // T, T, os.environ.get('DISTR_COMPACT32', '(default)')))
    _, st = functions.debug_tile_timing(eng, lat, pts[:nst], T)
    st = st.cpu().numpy().astype(np.int64)
    cyc, wall = st[:, :, 0], st[:, :, 1]
    d = np.median(cyc[:, 1:19] - cyc[:, 0:18], axis=0)
    tot_c, tot_w = np.median(cyc[:, 18] - cyc[:, 0]), np.median(wall[:, 18] - wall[:, 0])
    print('tile total %.0f cycles = %.1f us (clock %.3f GHz)' % (tot_c, tot_w / 100.0, tot_c / (tot_w * 10.0) if tot_w else 0))
    names = ['L%d %s' % (l, w) for l in range(8) for w in ('mfma', 'wb')] + ['lin8', 'end']
    print(' '.join('%s:%.0f' % (nm, v) for nm, v in zip(names, d)))
    ntile = min(64, args.n // T)
    fr = []
    layer_dump = functions.debug_mlp_layer if T == 64 else functions.debug_mlp_layer32
    for l in range(7):
        a = layer_dump(eng, lat, pts[:ntile * T], l).reshape(ntile, T, 512)[:, :, :253 if l == 3 else 512]
        fr.append(float((a > 0).any(dim=1).float().mean()))
    print('live fraction per layer (%d tiles): ' % ntile + ' '.join('L%d:%.3f' % (l, v) for l, v in enumerate(fr)))


if __name__ == '__main__':
    main()
