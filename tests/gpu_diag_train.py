"""Decoder-training timing (not a pytest file): forward + backward of decode_sdf_train (the layer-wise path) against
autograd through the torch Decoder in f32 on the same GPU (rocBLAS GEMMs, the (n, C + 3) input materialised), at 64 segments x 16 384
points and at 8 x 2 048. Every figure is the median of 5 hipEvent-bracketed runs after a warm-up run; the five samples are printed too.
The bracket is the whole call as a user makes it: weights on the autograd graph, the kernels, the loss reduction, backward to the
parameters and the codes.
    python tests/gpu_diag_train.py [--small]        --small: the 8 x 2 048 case only
Then the time per GEMM form (forward X W^T, delta Delta W, weights Delta^T X) from one profiled forward + backward (torch.profiler's
kernel table), as TFLOP/s of the layer arithmetic 2 * rows * (5 * 512^2 + 2 * 512 * (509 - C) + 512) per form."""
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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--small', action='store_true')
    args = ap.parse_args()
    from core.graph.deep_sdf_decoder import Decoder
    from core.utils.decoder_utils import decode_sdf_train
    from distr import fixture, functions
    Cn = 256
    Ws, bs, latent = fixture.make_decoder_weights()
    dec = Decoder(Cn, [512] * 8, norm_layers=(), latent_in=[4])
    dec.load_state_dict({('lin%d.%s' % (l, n)): torch.from_numpy(a) for l, (W, b) in enumerate(zip(Ws, bs)) for n, a in (('weight', W), ('bias', b))})
    dec = dec.cuda().eval()
    rs = np.random.RandomState(0)
    for S, N in ((8, 2048),) if args.small else ((8, 2048), (64, 16384)):
        lat0 = torch.from_numpy((latent + 0.3 * np.abs(latent).max() * rs.standard_normal((S, Cn))).astype(np.float32)).cuda()
        x0 = torch.from_numpy(((rs.rand(S, N, 3) - 0.5) * 1.6).astype(np.float32)).cuda()
        rows = functions.train_segment_rows([N] * S)[-1]
        flops = 2.0 * rows * (5 * 512 * 512 + 2 * 512 * (509 - Cn) + 512)

        def zero():
            for p in dec.parameters():
                p.grad = None

        def ours():
            zero()
            lat = lat0.clone().requires_grad_(True)
            decode_sdf_train(dec, lat, x0, clamp_dist=0.1).abs().sum().backward()
            return lat.grad

        def reference():
            zero()
            lat = lat0.clone().requires_grad_(True)
            inp = torch.cat([lat[:, None, :].expand(S, N, Cn).reshape(-1, Cn), x0.reshape(-1, 3)], 1)
            torch.clamp(dec(inp), -0.1, 0.1).abs().sum().backward()
            return lat.grad
        ga, gb = ours(), reference()
        print('S = %d x %d points: code gradient, decode_sdf_train against torch autograd: %.3e of its largest entry'
              % (S, N, ((ga - gb).abs().max() / gb.abs().max()).item()), flush=True)
        t_ref = timed(reference)
        print('S = %d x %d points, fwd+bwd: torch Decoder autograd (f32, rocBLAS) %.3f ms (%s)' % ((S, N) + t_ref), flush=True)
        t_our = timed(ours)
        print('S = %d x %d points, fwd+bwd: decode_sdf_train %.3f ms (%s); %.2f TFLOP/s over the three GEMM forms' % ((S, N) + t_our + (3 * flops / t_our[0] * 1e-9,)), flush=True)
        try:
            from torch.profiler import ProfilerActivity, profile
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                ours()
                torch.cuda.synchronize()
            per = {}
            for e in prof.key_averages():
                if 'k_train' in e.key:
                    us = getattr(e, 'device_time_total', None)
                    if us is None:
                        us = e.cuda_time_total
                    per[e.key] = (us, e.count)
            total = sum(v[0] for v in per.values())
            for k in sorted(per, key=lambda k: -per[k][0]):
                us, cnt = per[k]
                form = {'<true, true, 0>': 'forward X W^T', '<true, false, 1>': 'delta Delta W', '<false, false, 2>': 'weights Delta^T X'}
                name = [v for f, v in form.items() if f in k]
                extra = '  = %s: %.2f TFLOP/s' % (name[0], flops / us * 1e-6) if name else ''
                print('    %9.1f us %5.1f %% x%-3d %s%s' % (us, 100.0 * us / total, cnt, k.replace('distr::train::', '')[:90], extra), flush=True)
        except Exception as e:          # the kernel table is a convenience; the timings above stand without it
            print('    (no per-kernel table: %s: %s)' % (type(e).__name__, e), flush=True)
        del x0, lat0
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
