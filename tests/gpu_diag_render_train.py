"""Weight gradients through render, timing (not a pytest file): SDFRenderer.render forward + backward with and without decoder_grad, and
torch autograd through the torch Decoder on the same exported sample list for scale. Every figure is the median of 5 hipEvent-bracketed
runs after a warm-up run; the five samples are printed too (their spread is the yardstick for "moved"). The bracket is the whole call as
a user makes it: render, the loss, backward, and the Python between them.
    python tests/gpu_diag_render_train.py                  this build
    python tests/gpu_diag_render_train.py --tree PATH      another built checkout's dist-renderer_amd/ (the parent commit's: it has no
                                                           decoder_grad, so only the flag-off rows are measured -- the path that must not move)
  137 x 137 / 100 steps and 512 x 512 / 50 steps, pyramid_recursive, normals from depth, buffer 3, fixture F1, a dense loss on depth, normal
  and min_sdf."""
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
    import inspect
    from core.graph.deep_sdf_decoder import Decoder
    from core.sdfrenderer import SDFRenderer
    from distr import fixture, functions
    import distr
    assert os.path.abspath(distr.__file__).startswith(TREE + os.sep), (distr.__file__, TREE)      # the package measured is the one named
    tag = 'tree %s' % TREE if ARGS.tree else 'this build'
    has_flag = 'decoder_grad' in inspect.signature(SDFRenderer.__init__).parameters
    Ws, bs, latent = fixture.make_decoder_weights()
    dec = Decoder(256, [512] * 8, norm_layers=(), latent_in=[4])
    dec.load_state_dict({('lin%d.%s' % (l, n)): torch.from_numpy(a) for l, (W, b) in enumerate(zip(Ws, bs)) for n, a in (('weight', W), ('bias', b))})
    dec = dec.cuda().eval()
    R, T = fixture.make_camera(30, 20, 1.6, 10)
    lat0, R0, T0 = (torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda() for a in (latent, R, T))
    for size, steps in ((137, 100), (512, 50)):
        ren = SDFRenderer(dec, fixture.make_intrinsic(size, size), img_hw=(size, size), march_step=steps, buffer_size=3, use_depth2normal=True)
        rs = np.random.RandomState(size)
        wd, wq, wn = (torch.from_numpy(rs.rand(*s).astype(np.float32)).cuda() for s in ((size, size), (size, size), (size, size, 3)))

        def step():
            for p in dec.parameters():
                p.grad = None
            lat, Rt, Tt = (t.clone().requires_grad_(True) for t in (lat0, R0, T0))
            depth, normal, mask, q = ren.render(lat, Rt, Tt)
            ((depth * wd)[mask.bool()].sum() + (q * wq).sum() + (normal * wn).sum()).backward()
            return lat.grad
        if has_flag:
            ren.decoder_grad = False
        print('[%s] %d x %d / %d steps, render fwd+bwd, decoder_grad off: %.3f ms (%s)' % ((tag, size, size, steps) + timed(step)), flush=True)
        if not has_flag:
            continue
        ren.decoder_grad = True
        print('[%s] %d x %d / %d steps, render fwd+bwd, decoder_grad on:  %.3f ms (%s)' % ((tag, size, size, steps) + timed(step)), flush=True)
        # for scale: torch autograd through the torch Decoder over the same list (exported once, outside the bracket)
        from distr import binding
        eng = ren._engine
        lat, Rt, Tt = (t.clone().requires_grad_(True) for t in (lat0, R0, T0))
        cfg = ren._cfg(0.1, 'pyramid_recursive', True, want_normal=True)
        out = functions.render_batch_call(eng, cfg, lat, Rt[None], Tt[None])
        node = out[2].grad_fn
        P = size * size
        ws_b = torch.empty(eng.ctx.workspace_bytes(node.cfg)[1], dtype=torch.uint8, device='cuda')
        g_lat, g_R, g_T = torch.empty(1, 256, device='cuda'), torch.empty(1, 9, device='cuda'), torch.empty(1, 3, device='cuda')
        p = binding.ptr
        import ctypes as C
        gd = (wd * out[1].reshape(size, size).float()).contiguous()
        eng.ctx.check(eng.ctx.L.distr_render_backward_batch(eng.ctx.h, C.byref(node.cfg), 1, p(node.ws), node.ws.numel(), None, p(wq), p(gd), p(wn), p(g_lat), p(g_R),
                                                            p(g_T), p(ws_b), ws_b.numel(), eng.ctx.stream()))
        xyz, coef, _, counts = functions.render_samples(eng, node.cfg, node.ws, ws_b, 1)
        n = int(counts.cpu()[0])
        pts, cf = xyz[0, :n].contiguous(), coef[0, :n].contiguous()
        print('[%s] %d x %d: %d gradient samples of %d pixels; train workspace %.1f MB' % (tag, size, size, n, P, functions.train_plan_bytes([n]) / 2 ** 20), flush=True)

        def torch_autograd():
            for q_ in dec.parameters():
                q_.grad = None
            y = dec.inference(torch.cat([lat0.expand(n, -1), pts], 1))
            (y.reshape(-1) * cf).sum().backward()

        def train_path():
            weights = [q_.detach() for q_ in [dec.lin0.weight, dec.lin1.weight, dec.lin2.weight, dec.lin3.weight, dec.lin4.weight, dec.lin5.weight, dec.lin6.weight,
                                             dec.lin7.weight, dec.lin8.weight] + [getattr(dec, 'lin%d' % l).bias for l in range(9)]]
            _, saved = functions.train_forward(weights, lat0, pts, [n])
            functions.train_backward(saved, cf)
        print('[%s] %d x %d: torch autograd through the torch Decoder over the list: %.3f ms (%s)' % ((tag, size, size) + timed(torch_autograd)), flush=True)
        print('[%s] %d x %d: train_forward + train_backward over the list:           %.3f ms (%s)' % ((tag, size, size) + timed(train_path)), flush=True)


if __name__ == '__main__':
    main()
