"""Many-codes timing (not a pytest file): forward + backward of the decoder on S point lists with a code each, three ways, and the
single-code paths that must not get slower. Every figure is the median of 5 hipEvent-bracketed runs after a warm-up run; the five
samples are printed too (their spread is the yardstick for "slower"). The bracket is the whole call as a user makes it, end to end:
the kernels, and also the clones and requires_grad_ of the inputs, the loss reduction and the Python between them.
    python tests/gpu_diag_multi_code.py                  this build
    python tests/gpu_diag_multi_code.py --tree PATH      another built checkout's dist-renderer_amd/ (the parent commit's: it has no
                                                         decode_sdf_batch, so the batched rows are left out, and get_samples_batch and
                                                         decode_sdf show the parent's cost)
  A  S = 16 x 8192 and S = 64 x 2048 points: one decode_sdf_batch call against the loop of S decode_sdf calls
  B  get_samples_batch at 137^2, 8 views, a code per view
  C  decode_sdf forward + backward, one code, 8192 and 100000 points"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
_ap.add_argument('--tree', default=None, help="another built checkout's dist-renderer_amd/ to measure instead of this one's")
ARGS = _ap.parse_known_args()[0]          # before the package is imported: --tree decides which one that is
TREE = os.path.abspath(ARGS.tree) if ARGS.tree else os.path.join(ROOT, 'dist-renderer_amd')
sys.path.insert(0, TREE)
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


def main():
    from core.graph.deep_sdf_decoder import Decoder
    from core.sdfrenderer import SDFRenderer_deepsdf
    from core.utils import decoder_utils
    from distr import fixture
    decode_sdf, decode_sdf_batch = decoder_utils.decode_sdf, getattr(decoder_utils, 'decode_sdf_batch', None)
    batched = decode_sdf_batch is not None
    import distr
    assert os.path.abspath(distr.__file__).startswith(TREE + os.sep), (distr.__file__, TREE)      # the package measured is the one named
    tag = 'tree %s' % TREE if ARGS.tree else 'this build'
    Ws, bs, latent = fixture.make_decoder_weights()
    dec = Decoder(256, [512] * 8, norm_layers=(), latent_in=[4])
    dec.load_state_dict({('lin%d.%s' % (l, n)): torch.from_numpy(a) for l, (W, b) in enumerate(zip(Ws, bs)) for n, a in (('weight', W), ('bias', b))})
    dec = dec.cuda().eval()
    rs = np.random.RandomState(0)

    def codes(S):
        return torch.from_numpy((latent + 0.3 * np.abs(latent).max() * rs.standard_normal((S, 256))).astype(np.float32)).cuda()

    # A: S codes, one call against S calls
    for S, N in ((16, 8192), (64, 2048)):
        lat0, x0 = codes(S), torch.from_numpy(((rs.rand(S, N, 3) - 0.5) * 1.6).astype(np.float32)).cuda()

        def one_call():
            lat, x = lat0.clone().requires_grad_(True), x0.clone().requires_grad_(True)
            decode_sdf_batch(dec, lat, x).abs().sum().backward()
            return lat.grad

        def loop():
            lat, x = lat0.clone().requires_grad_(True), x0.clone().requires_grad_(True)
            sum(decode_sdf(dec, lat[s:s + 1], x[s]).abs().sum() for s in range(S)).backward()
            return lat.grad
        t_loop = timed(loop)
        print('A [%s] S = %d x %d points, fwd+bwd: loop of decode_sdf %.3f ms (%s)' % ((tag, S, N) + t_loop), flush=True)
        if batched:
            assert torch.equal(one_call(), loop())
            print('A [%s] S = %d x %d points, fwd+bwd: one decode_sdf_batch %.3f ms (%s)' % ((tag, S, N) + timed(one_call)), flush=True)

    # B: get_samples_batch, 8 views of 137^2 with a code each
    size, V = 137, 8
    ren = SDFRenderer_deepsdf(dec, fixture.make_intrinsic(size, size), img_hw=(size, size))
    lat0 = torch.from_numpy(latent).cuda() * torch.linspace(0.9, 1.1, V, device='cuda')[:, None]      # V shapes the views can see
    RTs, depths, normals = [], [], []
    for v in range(V):
        R, T = fixture.make_camera(20 + 40 * v, 20, 1.6, 10)
        Rt, Tt = torch.from_numpy(R).float().cuda(), torch.from_numpy(T).float().cuda()
        with torch.no_grad():
            d, n = ren.render(lat0[v:v + 1], Rt, Tt)[:2]
        RTs.append(torch.cat([Rt, Tt.reshape(3, 1)], 1)); depths.append(d.detach()); normals.append(n.detach())
    RT0, depth, normal = torch.stack(RTs), torch.stack(depths), torch.stack(normals)
    nvalid = int(((depth > 0) & (depth < 1e5)).sum())
    eta_map = torch.rand(nvalid, device='cuda') * 0.01

    def samples():
        lat, RT = lat0.clone().requires_grad_(True), RT0.clone().requires_grad_(True)
        out = ren.get_samples_batch(lat, RT, depth, normal, eta_map=eta_map)
        sum(p.abs().mean() + n.abs().mean() for p, n in out).backward()
        return lat.grad
    print('B [%s] get_samples_batch %d views of %d^2 (%d valid pixels), a code per view, fwd+bwd: %.3f ms (%s)'
          % ((tag, V, size, nvalid) + timed(samples)), flush=True)

    # C: the single-code path
    for N in (8192, 100000):
        lat0, x0 = codes(1), torch.from_numpy(((rs.rand(N, 3) - 0.5) * 1.6).astype(np.float32)).cuda()

        def single():
            lat, x = lat0.clone().requires_grad_(True), x0.clone().requires_grad_(True)
            decode_sdf(dec, lat, x).abs().sum().backward()
            return lat.grad
        print('C [%s] decode_sdf %d points, one code, fwd+bwd: %.3f ms (%s)' % ((tag, N) + timed(single)), flush=True)


if __name__ == '__main__':
    main()
