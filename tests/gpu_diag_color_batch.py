"""Textured-render timing (not a pytest file): SDFRenderer_color.render_batch against the loop of render calls it replaces, and relight
against lit render calls, at the settings of the reference's demos (100 march steps, buffer_size 1, ray_marching_ratio 1.0). Every
figure is the median of 5 hipEvent-bracketed runs after a warm-up run; the five samples are printed too. The bracket is the whole call
as a user makes it, forward only (the demos render without gradients).
    python tests/gpu_diag_color_batch.py [--sizes 1024 137]
  A  8 views of one shape: one render_batch against 8 render calls
  B  16 relit frames of one view: one relight against 16 lit render calls (and against one lit render_batch of 16 copies of the view)"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'dist-renderer_amd'))
import numpy as np
import torch


def timed(fn, reps=5):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), ' '.join('%.3f' % t for t in ts)


def module(Ws, bs, latent, dims, last):
    from core.graph.deep_sdf_decoder import Decoder
    d = Decoder(latent, dims, last_dim=last, norm_layers=(), latent_in=[4])
    d.load_state_dict({('lin%d.%s' % (l, n)): torch.from_numpy(a) for l, (W, b) in enumerate(zip(Ws, bs)) for n, a in (('weight', W), ('bias', b))})
    return d.cuda().eval()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--sizes', type=int, nargs='+', default=[1024, 137])
    args = ap.parse_args()
    from core.sdfrenderer import SDFRenderer_color
    from distr import fixture
    cs, V, F = 32, 8, 16
    Ws, bs, latent = fixture.make_decoder_weights()
    Wc, bc, code = fixture.make_color_decoder_weights(color_size=cs)
    dims_c = [512] * 8
    dims_c[3] += cs
    dec, dec_c = module(Ws, bs, 256, [512] * 8, 1), module(Wc, bc, 256 + cs, dims_c, 3)
    lat, cc = torch.from_numpy(latent).cuda(), torch.from_numpy(code).cuda()
    cams = [fixture.make_camera(20 + 40 * v, 20, 1.6, 10) for v in range(V)]
    Rs = torch.stack([torch.from_numpy(R).float() for R, _ in cams]).cuda()
    Ts = torch.stack([torch.from_numpy(T).float() for _, T in cams]).cuda()
    ang = torch.linspace(0, 2 * np.pi, F + 1)[:F]
    lights = torch.stack([2.5 * torch.cos(ang), torch.full_like(ang, 1.5), 2.5 * torch.sin(ang)], 1).reshape(F, 1, 3).cuda()
    for size in args.sizes:
        r = SDFRenderer_color(dec, dec_c, fixture.make_intrinsic(size, size), img_hw=(size, size), march_step=100, buffer_size=1,
                              ray_marching_ratio=1.0)
        with torch.no_grad():
            nvalid = int(r.render_batch(cc, lat, Rs, Ts, no_grad=True)[3].sum())

            def batch():
                return r.render_batch(cc, lat, Rs, Ts, no_grad=True)[2]

            def loop():
                return [r.render(cc, lat, Rs[v], Ts[v], no_grad=True)[2] for v in range(V)]
            print('A %d^2, %d views (%d valid pixels): %d render calls %.3f ms (%s)' % ((size, V, nvalid, V) + timed(loop)), flush=True)
            print('A %d^2, %d views (%d valid pixels): one render_batch %.3f ms (%s)' % ((size, V, nvalid) + timed(batch)), flush=True)
            d, n, col, m, q = r.render_batch(cc, lat, Rs[:1], Ts[:1], no_grad=True)
            z = r.render_depth(lat, Rs[0], Ts[0], no_grad=True)[0]

            def relight():
                return r.relight(col[0], n[0], z, m[0], Rs[0], Ts[0], lights)

            def lit_loop():
                return [r.render(cc, lat, Rs[0], Ts[0], no_grad=True, lighting_locations=lights[f])[2] for f in range(F)]

            def lit_batch():
                return r.render_batch(cc, lat, Rs[:1].expand(F, -1, -1), Ts[:1].expand(F, -1), no_grad=True, lighting_locations=lights)[2]
            print('B %d^2, %d relit frames: %d lit render calls %.3f ms (%s)' % ((size, F, F) + timed(lit_loop)), flush=True)
            print('B %d^2, %d relit frames: one lit render_batch of %d copies %.3f ms (%s)' % ((size, F, F) + timed(lit_batch)), flush=True)
            print('B %d^2, %d relit frames: one render_batch (B = 1) + one relight %.3f ms (%s)'
                  % ((size, F) + timed(lambda: (r.render_batch(cc, lat, Rs[:1], Ts[:1], no_grad=True), relight()))), flush=True)
            print('B %d^2, %d relit frames: relight alone %.3f ms (%s)' % ((size, F) + timed(relight)), flush=True)


if __name__ == '__main__':
    main()
