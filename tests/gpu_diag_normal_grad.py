"""Cost of normal_decoder_grad (not a pytest file): the backward pass of a render with a depth + normal + silhouette loss on raw
autograd normals, with and without the option, at 137^2 / 100 steps and 512^2 / 50 steps (pyramid_recursive, buffer 3). Every figure is
the median of 5 hipEvent-bracketed backward passes after a warm-up; the five samples are printed too. The bracket is loss.backward() as
a user calls it: the loss's own backward, the render node's main backward and -- with the option -- the second call (one compaction plus
one decoder backward over the valid pixels), with the Python between them. The forward is outside the bracket.
    python tests/gpu_diag_normal_grad.py"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'dist-renderer_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np
import torch


def timed_backward(forward, reps=5):
    """forward() -> loss; times loss.backward() alone."""
    ts = []
    for i in range(reps + 1):
        loss = forward()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        loss.backward()
        b.record()
        b.synchronize()
        if i:
            ts.append(a.elapsed_time(b))
    return float(np.median(ts)), ' '.join('%.3f' % t for t in ts)


def main():
    import helpers
    from distr import binding, fixture, functions
    Ws, bs, latent = fixture.make_decoder_weights()
    eng = functions.engine_from_weights(Ws, bs, 0)
    dev = eng.device
    for size, steps in ((137, 100), (512, 50)):
        K = fixture.make_intrinsic(size, size)
        R, T = fixture.make_camera(30, 20, 1.6, 10)
        cfg = binding.make_cfg((size, size), K, march_step=steps, buffer_size=3, marcher='pyramid_recursive', use_depth2normal=False, normalize_normal=False)
        wd, wq, wn = (torch.from_numpy(a).to(dev) for a in helpers.loss_weights(size, size, 5))
        valid = [0]

        def forward(option):
            lat, Rt, Tt = (torch.from_numpy(np.asarray(x, np.float32)).to(dev).requires_grad_(True) for x in (latent, R, T))
            z, mask, q, depth, normal = functions.render_call(eng, cfg, lat, Rt, Tt, normal_decoder_grad=option)
            valid[0] = int(mask.sum())
            return (depth * wd)[mask.reshape(size, size).bool()].sum() + (q.reshape(size, size) * wq).sum() + (normal * wn).sum()
        off = timed_backward(lambda: forward(False))
        on = timed_backward(lambda: forward(True))
        print('%d^2 / %d steps, %d valid pixels: backward without the option %.3f ms (%s)' % ((size, steps, valid[0]) + off), flush=True)
        print('%d^2 / %d steps, %d valid pixels: backward with    the option %.3f ms (%s)   difference %.3f ms'
              % ((size, steps, valid[0]) + on + (on[0] - off[0],)), flush=True)


if __name__ == '__main__':
    main()
