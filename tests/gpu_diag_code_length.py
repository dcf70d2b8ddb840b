"""Code-length timing (not a pytest file): the same workloads with fixture decoders of code length 256, 128 and 64 (narrow against wide layout), alternated
round by round so that clock drift hits every code length alike. Device events around synchronised work; median of the rounds.
    python tests/gpu_diag_code_length.py [rounds]
Workloads: 512^2 / 50 steps fwd + loss + bwd (bench.py C3: pyramid_recursive, buffer 3, depth2normal); 137^2 / 100 steps forward;
decode_sdf on 1 M points."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'dist-renderer_amd'), ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)
import numpy as np
import torch

CODE_LENGTHS = (256, 128, 64)


def event_ms(fn):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def main():
    import helpers
    from distr import binding, fixture, functions
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    dev = torch.device('cuda', 0)
    R, T = helpers.bench_camera(0)
    Rt, Tt = torch.from_numpy(R).to(dev), torch.from_numpy(T).to(dev)
    pts = ((torch.rand(1 << 20, 3, generator=torch.Generator().manual_seed(0)) - 0.5) * 1.6).to(dev)
    setups = {}
    for C in CODE_LENGTHS:
        Ws, bs, latent = fixture.make_decoder_weights(latent_size=C)
        setups[C] = (functions.engine_from_weights(Ws, bs, 0), torch.from_numpy(latent).to(dev))
    cfg512 = binding.make_cfg((512, 512), fixture.make_intrinsic(512, 512), march_step=50, buffer_size=3, marcher='pyramid_recursive',
                              use_depth2normal=True)
    cfg137 = binding.make_cfg((137, 137), fixture.make_intrinsic(137, 137), march_step=100, buffer_size=3, marcher='pyramid_recursive',
                              use_depth2normal=True)
    wd, wq, wn = (torch.from_numpy(a).to(dev) for a in helpers.loss_weights(512, 512, 5))

    def c3(eng, lat):
        lt = lat.clone().requires_grad_(True)
        zdepth, mask, q, depth, normal = functions.render_call(eng, cfg512, lt, Rt, Tt)
        L = (depth * wd)[mask.reshape(512, 512).bool()].sum() + (q.reshape(512, 512) * wq).sum() + (normal * wn).sum()
        L.backward()

    def fwd137(eng, lat):
        with torch.no_grad():
            functions.render_call(eng, cfg137, lat, Rt, Tt)

    def points(eng, lat):
        functions.mlp_eval(eng, lat, pts)

    work = (('512^2/50 fwd+bwd', c3), ('137^2/100 fwd', fwd137), ('decode_sdf 1M', points))
    res = {(w, C): [] for w, _ in work for C in CODE_LENGTHS}
    for C in CODE_LENGTHS:                       # warm-up (first launches, allocator)
        for _, fn in work:
            fn(*setups[C])
    for _ in range(rounds):
        for C in CODE_LENGTHS:
            for w, fn in work:
                res[(w, C)].append(event_ms(lambda: fn(*setups[C])))
    for w, _ in work:
        base = float(np.median(res[(w, 256)]))
        print('%-18s ' % w + '   '.join('C=%d %.3f ms (x%.3f)' % (C, float(np.median(res[(w, C)])), float(np.median(res[(w, C)])) / base)
                                         for C in CODE_LENGTHS), flush=True)


if __name__ == '__main__':
    main()
