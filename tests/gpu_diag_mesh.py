"""Shape-evaluation timing (not a pytest file): what the reference's Evaluator.latent_vec_to_points + compute_chamfer_distance do per
call (core/evaluation/transforms.py, eval_func.py), stage by stage, for N = 128 and 256 with the fixture decoder.
    python tests/gpu_diag_mesh.py"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'dist-renderer_amd'), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)
import numpy as np
import torch


def timed(fn, reps=5):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3, out


def main():
    from core.evaluation import create_sdf_grid_speedup
    from core.graph.deep_sdf_decoder import Decoder
    from distr import fixture, mesh
    Ws, bs, latent = fixture.make_decoder_weights()
    dec = Decoder(256, [512] * 8, norm_layers=(), latent_in=[4])
    dec.load_state_dict({('lin%d.%s' % (l, n)): torch.from_numpy(a) for l, (W, b) in enumerate(zip(Ws, bs)) for n, a in (('weight', W), ('bias', b))})
    dec = dec.cuda()
    lat = torch.from_numpy(latent).cuda()
    try:
        from scipy.spatial import cKDTree
    except ImportError:
        cKDTree = None
    for N in (128, 256):
        t_grid, grid = timed(lambda: create_sdf_grid_speedup(dec, lat, N))
        t_mc, (v, f) = timed(lambda: mesh.marching_cubes(grid, 0.0, voxel_size=2.0 / (N - 1)))
        t_s, (pts, _) = timed(lambda: mesh.sample_surface(v, f, 30000, seed=0))
        pts2, _ = mesh.sample_surface(v, f, 30000, seed=1)
        t_ch, ch = timed(lambda: mesh.chamfer(pts, pts2))
        line = ('N=%d: grid (speedup) %.2f ms | marching cubes %.2f ms (%d vertices, %d triangles) | sample 30000 %.3f ms | '
                'chamfer 30000 x 30000 %.3f ms (%.4e)' % (N, t_grid, t_mc, len(v), len(f), t_s, t_ch, ch))
        if cKDTree is not None:
            a, b = pts.cpu().numpy().astype(np.float64), pts2.cpu().numpy().astype(np.float64)

            def kd():
                one, _ = cKDTree(a).query(b)
                two, _ = cKDTree(b).query(a)
                return np.mean(np.square(one)) + np.mean(np.square(two))
            t_kd, ref = timed(kd, reps=3)
            line += ' | scipy cKDTree chamfer (host) %.1f ms (%.4e)' % (t_kd, ref)
        else:
            line += ' | scipy: not installed'
        print(line, flush=True)


if __name__ == '__main__':
    main()
