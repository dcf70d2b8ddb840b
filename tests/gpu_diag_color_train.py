"""Colour-decoder training timing (not a pytest file): forward + backward of decode_color_train (the layer-wise path on the colour net,
DESIGN.md section 8i) against autograd through the torch colour Decoder in f32 on the same GPU (rocBLAS GEMMs, the (n, 256 + cs + 3)
input materialised), cs = 256, loss |rgb - target|.mean(), at 8 segments x 2 048 points and at 64 x 16 384. Every figure is the median of
5 hipEvent-bracketed runs after a warm-up run; the five samples are printed too. The bracket is the whole call as a user makes it:
weights on the autograd graph, the kernels, the loss, backward to the parameters and both codes.
    python tests/gpu_diag_color_train.py [--small]        --small: the 8 x 2 048 case only"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'dist-renderer_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
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
    import color_train_restatement as cr
    from core.utils.decoder_utils import decode_color_train
    from distr import fixture, functions
    cs = 256
    Ws, bs, cc0 = fixture.make_color_decoder_weights(color_size=cs)
    dec = cr.color_module(Ws, bs, dtype=torch.float32).cuda()
    rs = np.random.RandomState(0)
    for S, N in ((8, 2048),) if args.small else ((8, 2048), (64, 16384)):
        c0 = torch.from_numpy((cc0 + 0.1 * rs.standard_normal((S, cs))).astype(np.float32)).cuda()
        s0 = torch.from_numpy((0.1 * rs.standard_normal((S, 256))).astype(np.float32)).cuda()
        x0 = torch.from_numpy(((rs.rand(S, N, 3) - 0.5) * 1.6).astype(np.float32)).cuda()
        target = torch.from_numpy(rs.rand(S, N, 3).astype(np.float32) - 0.5).cuda()
        rows = functions.train_segment_rows([N] * S)[-1]
        flops = 2.0 * rows * (5 * 512 * 512 + 2 * 512 * 253 + 3 * 512)          # one GEMM form; the code and xyz columns are folded

        def zero():
            for p in dec.parameters():
                p.grad = None

        def ours():
            zero()
            cc, sc = c0.clone().requires_grad_(True), s0.clone().requires_grad_(True)
            (decode_color_train(dec, cc, sc, x0) - target).abs().mean().backward()
            return cc.grad, sc.grad

        def reference():
            zero()
            cc, sc = c0.clone().requires_grad_(True), s0.clone().requires_grad_(True)
            lat = torch.cat([sc, cc], 1)
            inp = torch.cat([lat[:, None, :].expand(S, N, 256 + cs).reshape(-1, 256 + cs), x0.reshape(-1, 3)], 1)
            (dec(inp).reshape(S, N, 3) - target).abs().mean().backward()
            return cc.grad, sc.grad
        (ga, gsa), (gb, gsb) = ours(), reference()
        print('S = %d x %d points: code gradients, decode_color_train against torch autograd: colour %.3e, shape %.3e of the largest entry'
              % (S, N, ((ga - gb).abs().max() / gb.abs().max()).item(), ((gsa - gsb).abs().max() / gsb.abs().max()).item()), flush=True)
        t_ref = timed(reference)
        print('S = %d x %d points, fwd+bwd: torch colour Decoder autograd (f32, rocBLAS) %.3f ms (%s)' % ((S, N) + t_ref), flush=True)
        t_our = timed(ours)
        print('S = %d x %d points, fwd+bwd: decode_color_train %.3f ms (%s); %.2f TFLOP/s over the three GEMM forms; %.2f x torch'
              % ((S, N) + t_our + (3 * flops / t_our[0] * 1e-9, t_ref[0] / t_our[0])), flush=True)
        del x0, target
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
