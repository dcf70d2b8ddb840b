"""Depth-samples timing (not a pytest file): one SDFRenderer_deepsdf.get_samples forward + backward at 137^2 and 224^2 with the fixture
decoder, against the same quantities composed from the helpers that already ship (get_camera_location, get_camera_rays,
generate_point_samples, inv_transform_points, decode_sdf under autograd). Median of 5 runs each.
    python tests/gpu_diag_depth_samples.py"""
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
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3


def main():
    from core.graph.deep_sdf_decoder import Decoder
    from core.sdfrenderer import SDFRenderer_deepsdf
    from core.utils.decoder_utils import decode_sdf
    from distr import fixture
    Ws, bs, latent = fixture.make_decoder_weights()
    dec = Decoder(256, [512] * 8, norm_layers=(), latent_in=[4])
    dec.load_state_dict({('lin%d.%s' % (l, n)): torch.from_numpy(a) for l, (W, b) in enumerate(zip(Ws, bs)) for n, a in (('weight', W), ('bias', b))})
    dec = dec.cuda().eval()
    for size in (137, 224):
        ren = SDFRenderer_deepsdf(dec, fixture.make_intrinsic(size, size), img_hw=(size, size))
        R, T = fixture.make_camera(30, 20, 1.6, 10)
        Rt, Tt = torch.from_numpy(R).float().cuda(), torch.from_numpy(T).float().cuda()
        with torch.no_grad():
            depth, normal = ren.render(torch.from_numpy(latent).cuda(), Rt, Tt)[:2]
        depth, normal = depth.detach(), normal.detach()
        N = int(((depth > 0) & (depth < 1e5)).sum())
        eta_map = torch.rand(N, device='cuda') * 0.01
        RT0 = torch.cat([Rt, Tt.reshape(3, 1)], 1)

        def fused():
            lat, RT = torch.from_numpy(latent).cuda().requires_grad_(True), RT0.clone().requires_grad_(True)
            pos, neg = ren.get_samples(lat, RT, depth, normal, eta_map=eta_map)
            (pos.abs().mean() + neg.abs().mean()).backward()
            return lat.grad, RT.grad

        def composed():
            lat, RT = torch.from_numpy(latent).cuda().requires_grad_(True), RT0.clone().requires_grad_(True)
            R_, T_ = RT[:, :3], RT[:, 3]
            cam_pos, rays = ren.get_camera_location(R_, T_), ren.get_camera_rays(R_)
            d = depth.reshape(-1)
            valid = (d > 0) & (d < 1e5)
            p = ren.generate_point_samples(cam_pos, rays[:, valid], d[valid] / ren.calib_map[valid]).t()
            off = ren.inv_transform_points(normal.reshape(-1, 3)[valid].t()).t() * eta_map[:, None]
            pos = decode_sdf(dec, lat, p + off, clamp_dist=0.1).squeeze(-1) - eta_map
            neg = decode_sdf(dec, lat, p - off, clamp_dist=0.1).squeeze(-1) + eta_map
            (pos.abs().mean() + neg.abs().mean()).backward()
            return lat.grad, RT.grad
        a, b = fused(), composed()
        print('%d^2: %d valid pixels; get_samples fwd+bwd %.3f ms, composed helpers %.3f ms (g_latent differ by %.2e relative)'
              % (size, N, timed(fused), timed(composed), float((a[0] - b[0]).abs().max() / b[0].abs().max())), flush=True)


if __name__ == '__main__':
    main()
