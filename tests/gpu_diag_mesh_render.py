"""Mesh render timing (not a pytest file): distr.mesh.render_mesh of the fixture decoder's N = 128 and N = 256 marching-cubes meshes at
137 x 137 x 8 views and 512 x 512 x 1 view, in ms (median of 3 host-timed calls that end in a device synchronise, after a warm-up) and
(ray, triangle) pairs per second. There is no earlier version to compare with; the yardstick is the same formulas composed from torch
operations on the same GPU, in chunks of 2^24 pairs, on TORCH_PIXELS pixels spread over the first view (it is too slow for all of them;
pairs per second is the comparable figure). The two must agree in mask and face on those pixels.
    python tests/gpu_diag_mesh_render.py"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'dist-renderer_amd'), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)
import numpy as np
import torch

TORCH_PIXELS = 2048
PAIRS_PER_STEP = 1 << 24
M = np.array([[1., 0., 0.], [0., 0., -1.], [0., 1., 0.]])


def timed(fn, reps=3):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3, out


def _dot(u, v):
    return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]


def _cross(p, q):
    return [p[1] * q[2] - p[2] * q[1], p[2] * q[0] - p[0] * q[2], p[0] * q[1] - p[1] * q[0]]


def torch_cast(v, f, K, RT, hw, pix):
    """csrc/distr_mesh.hpp's formulas (k_mesh_cast) from torch operations, float32, for the pixels `pix` of one view: (mask, face)."""
    dev = v.device
    Ki = torch.from_numpy(np.linalg.inv(K).astype(np.float32)).to(dev)
    Mt = torch.from_numpy(M.astype(np.float32)).to(dev)
    R, T = RT[:, :3], RT[:, 3]
    c = [-(R[0, i] * T[0] + R[1, i] * T[1] + R[2, i] * T[2]) for i in range(3)]
    o = [Mt[0, i] * c[0] + Mt[1, i] * c[1] + Mt[2, i] * c[2] for i in range(3)]
    x, y = (pix % hw[1]).float(), (pix // hw[1]).float()
    h = [Ki[a, 0] * x + Ki[a, 1] * y + Ki[a, 2] for a in range(3)]
    r = [R[0, i] * h[0] + R[1, i] * h[1] + R[2, i] * h[2] for i in range(3)]
    rn = torch.sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2])
    d = [r[i] / (rn + 1e-12) for i in range(3)]
    e = [Mt[0, i] * d[0] + Mt[1, i] * d[1] + Mt[2, i] * d[2] for i in range(3)]
    a, b, cc = v[f[:, 0].long()], v[f[:, 1].long()], v[f[:, 2].long()]
    ok = (torch.isfinite(a).all(1) & torch.isfinite(b).all(1) & torch.isfinite(cc).all(1) & ~(torch.linalg.cross(b - a, cc - a) == 0).all(1))[None, :]
    A, B, C = ([(p[:, k] - o[k])[None, :] for k in range(3)] for p in (a, b, cc))
    Na, Nb, Nc = _cross(C, B), _cross(A, C), _cross(B, A)
    Ng = _cross([B[k] - A[k] for k in range(3)], [C[k] - A[k] for k in range(3)])
    ANg = _dot(A, Ng)
    rows = max(1, PAIRS_PER_STEP // len(f))
    inf = torch.full((), float('inf'), device=dev)
    mask, face = [], []
    for i0 in range(0, len(pix), rows):
        eb = [z[i0:i0 + rows, None] for z in e]
        U, V, W = _dot(eb, Na), _dot(eb, Nb), _dot(eb, Nc)
        mixed = ((U < 0) | (V < 0) | (W < 0)) & ((U > 0) | (V > 0) | (W > 0))
        t = ANg / _dot(eb, Ng)
        t = torch.where(ok & ~mixed & (((U + V) + W) != 0) & torch.isfinite(t) & (t > 0), t, inf)
        best = t.min(1)
        hit = torch.isfinite(best.values)
        first = (t == best.values[:, None]).float().argmax(1)          # the lowest face among equal t
        mask.append(hit)
        face.append(torch.where(hit, first, torch.full_like(first, -1)))
    return torch.cat(mask), torch.cat(face)


def main():
    from core.evaluation import create_sdf_grid_speedup
    from core.graph.deep_sdf_decoder import Decoder
    from distr import fixture, mesh
    Ws, bs, latent = fixture.make_decoder_weights()
    dec = Decoder(256, [512] * 8, norm_layers=(), latent_in=[4])
    dec.load_state_dict({('lin%d.%s' % (l, n)): torch.from_numpy(a) for l, (W, b) in enumerate(zip(Ws, bs)) for n, a in (('weight', W), ('bias', b))})
    dec = dec.cuda()
    lat = torch.from_numpy(latent).cuda()
    for N in (128, 256):
        grid = create_sdf_grid_speedup(dec, lat, N)
        v, f = mesh.marching_cubes(grid, 0.0, voxel_size=2.0 / (N - 1))
        for (H, W), views in (((137, 137), 8), ((512, 512), 1)):
            K = fixture.make_intrinsic(H, W)
            cams = [fixture.make_camera(-60 + 40 * k, 10 + 5 * k, 1.5 + 0.05 * k, 6 * k) for k in range(views)]
            RT = torch.from_numpy(np.stack([np.concatenate([R, T[:, None]], 1) for R, T in cams]).astype(np.float32)).cuda()
            t_k, out = timed(lambda: mesh.render_mesh(v, f, K, RT, (H, W), details=True))
            pix = torch.linspace(0, H * W - 1, TORCH_PIXELS, device='cuda').long()
            t_t, (tm, tf) = timed(lambda: torch_cast(v, f, K, RT[0], (H, W), pix), reps=2)
            km, kf = out[2][0].reshape(-1)[pix].bool(), out[4][0].reshape(-1)[pix]
            pairs = H * W * views * len(f)
            print('N=%d: %d vertices, %d triangles | %d x %d x %d views: render_mesh %.2f ms = %.3g pairs/s, %.1f %% of the pixels hit | torch '
                  'composition, %d pixels of view 0: %.1f ms = %.3g pairs/s | kernel / torch %.1fx | on those: mask differs at %d, face at %d'
                  % (N, len(v), len(f), H, W, views, t_k, pairs / (t_k * 1e-3), 100.0 * float(out[2].float().mean()), len(pix), t_t,
                     len(pix) * len(f) / (t_t * 1e-3), (pairs / t_k) / (len(pix) * len(f) / t_t), int((km != tm).sum()), int((kf != tf).sum())),
                  flush=True)
            assert bool((km == tm).all()) and bool((kf == tf).all()), 'kernel and torch composition disagree'


if __name__ == '__main__':
    main()
