"""Signed-distance timing (not a pytest file): 500 000 queries against the fixture decoder's N = 128 and N = 256 marching-cubes meshes
with distr.mesh.signed_distance, in ms and (query, triangle) pairs per second. There is no earlier version to compare with; the
yardstick is the same formulas composed from torch operations on the same GPU, in chunks of 2^24 pairs, on the first TORCH_QUERIES
queries (it is too slow for all of them; pairs per second is the comparable figure). Also prints how far the two agree.
    python tests/gpu_diag_mesh_sdf.py"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'dist-renderer_amd'), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)
import numpy as np
import torch

QUERIES = 500000
TORCH_QUERIES = 4096
PAIRS_PER_STEP = 1 << 24


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


def torch_signed_distance(v, f, Q):
    """csrc/distr_mesh.hpp's formulas (k_sdf_pairs) from torch operations, float32, float64 sum of the solid angles: (sdf, dist2, w)."""
    a, b, c = v[f[:, 0].long()], v[f[:, 1].long()], v[f[:, 2].long()]
    ab, ac = b - a, c - a
    cr = torch.linalg.cross(ab, ac)
    ok = (torch.isfinite(a).all(1) & torch.isfinite(b).all(1) & torch.isfinite(c).all(1) & ~(cr == 0).all(1))[None, :]
    a_, ab_, ac_ = ([x[None, :, k] for k in range(3)] for x in (a, ab, ac))
    one, zero = torch.ones((), device=v.device), torch.zeros((), device=v.device)
    rows = max(1, PAIRS_PER_STEP // len(f))
    out = []
    for i0 in range(0, len(Q), rows):
        q = [Q[i0:i0 + rows, k, None] for k in range(3)]
        ap = [q[k] - a_[k] for k in range(3)]
        bp = [ap[k] - ab_[k] for k in range(3)]
        cp = [ap[k] - ac_[k] for k in range(3)]
        d1, d2, d3, d4, d5, d6 = _dot(ab_, ap), _dot(ac_, ap), _dot(ab_, bp), _dot(ac_, bp), _dot(ab_, cp), _dot(ac_, cp)
        vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
        e43, e56 = d4 - d3, d5 - d6
        sd = (va + vb) + vc
        sn, tn, td = vb, vc, sd
        bc = (va <= 0) & (e43 >= 0) & (e56 >= 0)
        for cond, vals in ((bc, (one, one, e43, e43 + e56)),
                           ((vb <= 0) & (d2 >= 0) & (d6 <= 0), (zero, one, d2, d2 - d6)),
                           ((d6 >= 0) & (d5 <= d6), (zero, one, one, one)),
                           ((vc <= 0) & (d1 >= 0) & (d3 <= 0), (d1, d1 - d3, zero, one)),
                           ((d3 >= 0) & (d4 <= d3), (one, one, zero, one)),
                           ((d1 <= 0) & (d2 <= 0), (zero, one, zero, one))):
            sn, sd, tn, td = (torch.where(cond, x, y) for x, y in zip(vals, (sn, sd, tn, td)))
            if cond is not bc:
                bc = bc & ~cond
        s, t = sn / sd, tn / td
        e = [torch.where(bc, ac_[k] - ab_[k], ac_[k]) for k in range(3)]
        d = [q[k] - ((a_[k] + s * ab_[k]) + t * e[k]) for k in range(3)]
        dist2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
        dist2 = torch.where(ok & (dist2 < float('inf')), dist2, torch.full_like(dist2, float('inf')))
        A = [a_[k] - q[k] for k in range(3)]
        B = [A[k] + ab_[k] for k in range(3)]
        Cc = [A[k] + ac_[k] for k in range(3)]
        num = _dot(A, [B[1] * Cc[2] - B[2] * Cc[1], B[2] * Cc[0] - B[0] * Cc[2], B[0] * Cc[1] - B[1] * Cc[0]])
        la, lb, lc = torch.sqrt(_dot(A, A)), torch.sqrt(_dot(B, B)), torch.sqrt(_dot(Cc, Cc))
        den = ((((la * lb) * lc) + _dot(A, B) * lc) + _dot(B, Cc) * la) + _dot(Cc, A) * lb
        half = torch.where(ok, torch.atan2(num, den), zero)
        w = (half.sum(1, dtype=torch.float64) * 0.15915494309189535).float()
        best = dist2.min(1).values
        out.append((torch.where(w.abs() > 0.5, -one, one) * best.sqrt(), best, w))
    return tuple(torch.cat(x) for x in zip(*out))


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
        pts, _ = mesh.sample_surface(v, f, QUERIES // 2, seed=0)
        q = mesh.sdf_queries(pts, (0.005 ** 0.5, 0.0005 ** 0.5), QUERIES - 2 * (QUERIES // 2), 1.0, 0)[:QUERIES].contiguous()
        t_q, _ = timed(lambda: mesh.sdf_queries(pts, (0.005 ** 0.5, 0.0005 ** 0.5), 0, 1.0, 0))
        t_k, (sdf, d2, w, _) = timed(lambda: mesh.signed_distance(v, f, q, details=True))
        t_t, (tsdf, td2, tw) = timed(lambda: torch_signed_distance(v, f, q[:TORCH_QUERIES]), reps=2)
        n = TORCH_QUERIES
        rel = float(((d2[:n] - td2).abs() / td2.clamp_min(1e-30)).max())
        print('N=%d: %d vertices, %d triangles | %d queries: generate %.3f ms, signed_distance %.1f ms = %.3g pairs/s | torch composition, '
              '%d queries: %.1f ms = %.3g pairs/s | kernel / torch %.1fx | agreement on those: dist2 max rel %.2g, winding max abs %.2g, '
              'signs differ at %d | inside %.1f %%'
              % (N, len(v), len(f), len(q), t_q, t_k, len(q) * len(f) / (t_k * 1e-3), n, t_t, n * len(f) / (t_t * 1e-3),
                 (n * len(f) / t_t) and (len(q) * len(f) / t_k) / (n * len(f) / t_t), rel, float((w[:n] - tw).abs().max()),
                 int(((sdf[:n] < 0) != (tsdf < 0)).sum()), 100.0 * float((sdf < 0).float().mean())), flush=True)


if __name__ == '__main__':
    main()
