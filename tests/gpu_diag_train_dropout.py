"""Timing of dropout on the layer-wise train path (not a pytest file): forward + backward of decode_sdf_train with
dropout on all eight layers (p = 0.2, a fresh seed per run as in training) and without it, in the same process, and autograd through
the torch Decoder in training mode (f32, rocBLAS GEMMs, F.dropout) on the same GPU; C = 256, at 8 x 2 048 and 64 x 16 384 points.
Every figure is the median of 5 hipEvent-bracketed runs after a warm-up run; the five samples are printed too. The bracket is the
whole call as a user makes it (weights on the autograd graph, the kernels, the loss reduction, backward to the parameters and codes).
    python tests/gpu_diag_train_dropout.py [--small]        --small: the 8 x 2 048 case only
Each size runs in a process of its own under `timeout`; the first one that fails ends the script. Then the kernels of one profiled
forward + backward with dropout (torch.profiler's kernel table)."""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'dist-renderer_amd'))
CASES = ((8, 2048, 120), (64, 16384, 300))         # segments, points per segment, time limit of the step (s)


def timed(fn, reps=5):
    import numpy as np
    import torch
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


def run_case(S, N):
    import numpy as np
    import torch
    from core.graph.deep_sdf_decoder import Decoder
    from core.utils.decoder_utils import decode_sdf_train
    from distr import fixture
    Cn = 256
    Ws, bs, latent = fixture.make_decoder_weights()
    dec = Decoder(Cn, [512] * 8, norm_layers=(), latent_in=[4], dropout=list(range(8)), dropout_prob=0.2)
    dec.load_state_dict({('lin%d.%s' % (l, n)): torch.from_numpy(a) for l, (W, b) in enumerate(zip(Ws, bs)) for n, a in (('weight', W), ('bias', b))})
    dec = dec.cuda()
    rs = np.random.RandomState(0)
    lat0 = torch.from_numpy((latent + 0.3 * np.abs(latent).max() * rs.standard_normal((S, Cn))).astype(np.float32)).cuda()
    x0 = torch.from_numpy(((rs.rand(S, N, 3) - 0.5) * 1.6).astype(np.float32)).cuda()
    seed = [0x5EED]

    def zero():
        for p in dec.parameters():
            p.grad = None

    def ours(drop):
        zero()
        dec.train(drop)
        seed[0] += 1
        lat = lat0.clone().requires_grad_(True)
        decode_sdf_train(dec, lat, x0, clamp_dist=None, dropout_seed=seed[0] if drop else None).abs().sum().backward()
        return lat.grad

    def reference():
        zero()
        dec.train()
        lat = lat0.clone().requires_grad_(True)
        inp = torch.cat([lat[:, None, :].expand(S, N, Cn).reshape(-1, Cn), x0.reshape(-1, 3)], 1)
        dec(inp).abs().sum().backward()
        return lat.grad
    tag = 'S = %d x %d points, fwd+bwd' % (S, N)
    t_off = timed(lambda: ours(False))
    print('%s: decode_sdf_train, eval mode (the path without dropout) %.3f ms (%s)' % ((tag,) + t_off), flush=True)
    t_on = timed(lambda: ours(True))
    print('%s: decode_sdf_train, dropout p = 0.2 on lin0..lin7        %.3f ms (%s)' % ((tag,) + t_on), flush=True)
    t_ref = timed(reference)
    print('%s: torch Decoder in training mode (f32, rocBLAS, F.dropout) %.3f ms (%s)' % ((tag,) + t_ref), flush=True)
    print('%s: dropout on / off = %.3f; torch / dropout on = %.3f' % (tag, t_on[0] / t_off[0], t_ref[0] / t_on[0]), flush=True)
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            ours(True)
            torch.cuda.synchronize()
        per = {}
        for e in prof.key_averages():
            if 'k_train' in e.key:
                us = getattr(e, 'device_time_total', None)
                per[e.key] = (e.cuda_time_total if us is None else us, e.count)
        total = sum(v[0] for v in per.values())
        for k in sorted(per, key=lambda k: -per[k][0]):
            print('    %9.1f us %5.1f %% x%-3d %s' % (per[k][0], 100.0 * per[k][0] / total, per[k][1], k.replace('distr::train::', '')[:100]), flush=True)
    except Exception as e:          # the kernel table is a convenience; the timings above stand without it
        print('    (no per-kernel table: %s: %s)' % (type(e).__name__, e), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--small', action='store_true')
    ap.add_argument('--case', nargs=2, type=int, metavar=('S', 'N'), help='run one size in this process')
    args = ap.parse_args()
    if args.case:
        run_case(*args.case)
        return 0
    for S, N, limit in CASES[:1] if args.small else CASES:
        rc = subprocess.call(['timeout', '-k', '10', str(limit), sys.executable, os.path.abspath(__file__), '--case', str(S), str(N)])
        if rc != 0:
            print('S = %d x %d: exit status %d; stopping here' % (S, N, rc), flush=True)
            return rc
    return 0


if __name__ == '__main__':
    sys.exit(main())
