"""Timing of training through the spatial gradient (not a pytest file): forward + backward of decode_sdf_gradient_train (DESIGN.md section
8m) with a loss on both outputs, mean((|g| - 1)^2) + mean|f|, against
  * decode_sdf_train on the same list (a loss on f alone: 24 GEMMs of the list's size against 40 here), and
  * torch autograd with create_graph=True through the torch Decoder in f32 on the same GPU (rocBLAS GEMMs, double backward),
at 8 segments x 2 048 points and at 64 x 16 384. Every figure is the median of 3 hipEvent-bracketed runs after a warm-up run; the
samples are printed too. The bracket is the whole call as a user makes it: weights on the autograd graph, the kernels, the loss,
backward to the parameters and the codes. Then the worst f32 residual of torch's own double backward and of this path against float64
autograd on the small case's first segment.
The large case needs a workspace of 40 GiB (40 KB per point), above the default DISTR_TRAIN_MAX_BYTES of 32 GiB: this script raises the
cap to 64 GiB unless the variable is set.
    python tests/gpu_diag_train_grad.py [--small]        --small: the 8 x 2 048 case only"""
import argparse
import copy
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'dist-renderer_amd'))
import numpy as np
import torch


def timed(fn, reps=3):
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


def loss_of(f, g):
    return ((g.norm(dim=-1) - 1) ** 2).mean() + f.abs().mean()


def torch_double_backward(dec, lat, x, S, N, Cn):
    """the loss through the torch Decoder: grad_x f by autograd.grad(create_graph=True), then backward -> (loss, parameter gradients)"""
    for p in dec.parameters():
        p.grad = None
    xr = x.reshape(-1, 3).clone().requires_grad_(True)
    y = dec(torch.cat([lat[:, None, :].expand(S, N, Cn).reshape(-1, Cn), xr], 1))
    g, = torch.autograd.grad(y.sum(), xr, create_graph=True)
    loss = loss_of(y, g)
    loss.backward()
    return loss


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--small', action='store_true')
    args = ap.parse_args()
    os.environ.setdefault('DISTR_TRAIN_MAX_BYTES', str(64 << 30))
    from core.graph.deep_sdf_decoder import Decoder
    from core.utils.decoder_utils import decode_sdf_gradient_train, decode_sdf_train
    from distr import fixture
    Cn = 256
    Ws, bs, latent = fixture.make_decoder_weights()
    dec = Decoder(Cn, [512] * 8, norm_layers=(), latent_in=[4])
    dec.load_state_dict({('lin%d.%s' % (l, n)): torch.from_numpy(a) for l, (W, b) in enumerate(zip(Ws, bs)) for n, a in (('weight', W), ('bias', b))})
    dec = dec.cuda().eval()
    rs = np.random.RandomState(0)
    for S, N in ((8, 2048),) if args.small else ((8, 2048), (64, 16384)):
        lat0 = torch.from_numpy((latent + 0.3 * np.abs(latent).max() * rs.standard_normal((S, Cn))).astype(np.float32)).cuda()
        x0 = torch.from_numpy(((rs.rand(S, N, 3) - 0.5) * 1.6).astype(np.float32)).cuda()

        def zero():
            for p in dec.parameters():
                p.grad = None

        def ours():
            zero()
            lat = lat0.clone().requires_grad_(True)
            f, g = decode_sdf_gradient_train(dec, lat, x0)
            loss_of(f, g).backward()
            return lat.grad

        def value_only():
            zero()
            lat = lat0.clone().requires_grad_(True)
            decode_sdf_train(dec, lat, x0, clamp_dist=None).abs().mean().backward()
            return lat.grad

        def reference():
            lat = lat0.clone().requires_grad_(True)
            torch_double_backward(dec, lat, x0, S, N, Cn)
            return lat.grad
        ga, gb = ours(), reference()
        print('S = %d x %d points: code gradient, decode_sdf_gradient_train against torch double backward (f32): %.3e of its largest entry'
              % (S, N, ((ga - gb).abs().max() / gb.abs().max()).item()), flush=True)
        t_val = timed(value_only)
        print('S = %d x %d points, fwd+bwd: decode_sdf_train (loss on f alone) %.3f ms (%s)' % ((S, N) + t_val), flush=True)
        t_our = timed(ours)
        print('S = %d x %d points, fwd+bwd: decode_sdf_gradient_train %.3f ms (%s); %.2f x decode_sdf_train' % ((S, N) + t_our + (t_our[0] / t_val[0],)), flush=True)
        try:
            t_ref = timed(reference)
            print('S = %d x %d points, fwd+bwd: torch Decoder double backward (f32, rocBLAS) %.3f ms (%s); %.2f x this path'
                  % ((S, N) + t_ref + (t_ref[0] / t_our[0],)), flush=True)
        except torch.cuda.OutOfMemoryError as e:
            print('S = %d x %d points: torch double backward does not fit: %s' % (S, N, str(e).split('.')[0]), flush=True)
        if (S, N) == (8, 2048):
            # what f32 costs on this term: both f32 paths against float64 autograd, one segment (the ReLU pattern is each run's own:
            # a unit that flips side shows up here, unlike in the tests, which hand the GPU's gates to the reference)
            d64 = copy.deepcopy(dec).double()
            lat64 = lat0[:1].double().clone().requires_grad_(True)
            torch_double_backward(d64, lat64, x0[:1].double(), 1, N, Cn)
            ref = [p.grad for p in d64.parameters()] + [lat64.grad]
            lat32 = lat0[:1].clone().requires_grad_(True)
            torch_double_backward(dec, lat32, x0[:1], 1, N, Cn)
            got_t = [p.grad.clone() for p in dec.parameters()] + [lat32.grad]
            zero()
            lat = lat0[:1].clone().requires_grad_(True)
            f, g = decode_sdf_gradient_train(dec, lat, x0[:1])
            loss_of(f, g).backward()
            got_o = [p.grad for p in dec.parameters()] + [lat.grad]
            rel = lambda got: max(((a.double() - b).abs().max() / b.abs().max()).item() for a, b in zip(got, ref))
            print('1 x %d points, Eikonal + L1 loss, worst tensor against float64 autograd: torch f32 double backward %.3e, this path %.3e of the largest entry'
                  % (N, rel(got_t), rel(got_o)), flush=True)
        del x0, lat0
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
