"""k-steps the compacted 64-ray forward tiles execute against the dense count, per march launch of one forward (not a pytest file): the
headline configuration by default (512 x 512, 50 steps, pyramid_recursive, buffer size 3, bench view 0, fixture F1). Reads the device
counter (Consts::kstep_fine / kstep_coarse through render_stats(ksteps=True)) and the live counts, and prints one line per launch that ran
compacted tiles, the sums over the coarse launches, over full-resolution steps 1..10 and over all rounds, and the launches of the forward.
DISTR_LIVE_ORDER=0|1 and DISTR_RAY_BLOCKS=0|1 in the environment choose the list order and the pixel enumeration (read at distr_create);
both at 0 is the behaviour before the ordered list.

    python profiles/tools/live_order_ksteps.py [--size 512] [--march-step 50] [--marcher pyramid_recursive] [--view 0] [--reps 3]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (os.path.join(ROOT, 'dist-renderer_amd'), ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)
import numpy as np
import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--march-step', type=int, default=50)
    ap.add_argument('--marcher', default='pyramid_recursive')
    ap.add_argument('--view', type=int, default=0)
    ap.add_argument('--reps', type=int, default=3, help='forwards rendered; the last one is reported (the tail launch starts where the previous render says)')
    args = ap.parse_args()
    import helpers
    from distr import binding, fixture, functions
    Ws, bs, latent = fixture.make_decoder_weights()
    eng = functions.engine_from_weights(Ws, bs, 0)
    dev = eng.device
    S = args.size
    K = fixture.make_intrinsic(S, S)
    R, T = helpers.bench_camera(args.view)
    cfg = binding.make_cfg((S, S), K, march_step=args.march_step, buffer_size=3, ratio=1.5, marcher=args.marcher, use_depth2normal=True)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev).requires_grad_(True)
    lat, Rt, Tt = t(latent), t(R), t(T)
    for _ in range(args.reps):
        out = functions.render_call(eng, cfg, lat, Rt, Tt)
    torch.cuda.synchronize()
    node = out[2].grad_fn
    while node is not None and not hasattr(node, 'ws'):
        node = node.next_functions[0][0]
    st = eng.ctx.render_stats(node.cfg, node.ws, ksteps=True)
    rays = eng.ctx.live_counts(node.cfg, node.ws)
    ks = st['ksteps']
    assert len(rays) == len(ks)      # (both lists are in launch order)
    fwd_bytes = eng.ctx.workspace_bytes(node.cfg)[0]
    print('DISTR_LIVE_ORDER=%s DISTR_RAY_BLOCKS=%s  %d x %d, %d steps, %s, view %d; forward workspace %d bytes' %
          (os.environ.get('DISTR_LIVE_ORDER', '1'), os.environ.get('DISTR_RAY_BLOCKS', '1'), S, S, args.march_step, args.marcher, args.view, fwd_bytes))
    print('march launches %d (tail launch from step %d), point evaluations %d' % (st['num_march_launches'], st['tail_from'], st['num_point_evals']))
    # the coarse levels' steps come first: the full-resolution steps are the last entries
    ncoarse = len(ks) - _fine_steps(node.cfg, len(ks))
    print('%-10s %9s %7s %10s %10s %6s' % ('launch', 'rays', 'tiles', 'k-steps', 'dense', 'kept'))
    groups = {'coarse': [0, 0], 'steps 1..10': [0, 0], 'all steps': [0, 0]}
    for i, ((tiles, done, dense), r) in enumerate(zip(ks, rays)):
        label = 'coarse %d' % i if i < ncoarse else 'step %d' % (i - ncoarse)
        if tiles:
            print('%-10s %9d %7d %10d %10d %6.3f' % (label, r, tiles, done, dense, done / dense))
        keys = ['coarse'] if i < ncoarse else (['all steps'] + (['steps 1..10'] if 1 <= i - ncoarse <= 10 else []))
        for k in keys:
            groups[k][0] += done
            groups[k][1] += dense
    for k, (done, dense) in groups.items():
        if dense:
            print('%-12s k-steps %11d of %11d dense: kept %.3f' % (k, done, dense, done / dense))


def _fine_steps(cfg, total):
    """Full-resolution steps of cfg: march_step minus the coarse levels' steps (the default pyramid: coarse_steps; `total` launches otherwise)."""
    from distr import binding
    if cfg.marcher != binding.MARCHERS['pyramid_recursive']:
        return total
    if cfg.num_levels:
        return int(cfg.march_step) - sum(int(cfg.level_steps[i]) for i in range(int(cfg.num_levels) - 1))
    return int(cfg.march_step) - int(cfg.coarse_steps[0]) - int(cfg.coarse_steps[1])


if __name__ == '__main__':
    main()
