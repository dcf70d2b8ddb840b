"""Weight gradients of the colour decoder through the colour render, timing (not a pytest file): SDFRenderer_color.render_batch of 8 views
at 137 x 137 / 100 steps with the loss mean |rgb - gt| + SSIM and backward, with and without color_decoder_grad, and the loss alone --
the fused one (compute_loss_color_batch) against the torch composition of the same formula. Every figure is the median of 5
hipEvent-bracketed runs after a warm-up run; the five samples are printed too (their spread is the yardstick for "moved"). The bracket
is the whole call as a user makes it: render_batch, the loss, backward, and the Python between them.
    python tests/gpu_diag_color_render_train.py                  this build
    python tests/gpu_diag_color_render_train.py --tree PATH      another built checkout's dist-renderer_amd/ (the parent commit's: it has
                                                                 no color_decoder_grad and no fused loss, so only the flag-off row with
                                                                 the torch loss is measured -- the path that must not move)
The render rows use the torch composition of the loss in every tree, so that they differ in the render path only; the last row of this
build swaps in the fused loss."""
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
import torch.nn.functional as F

B, SIZE, STEPS, CS = 8, 137, 100, 32


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


def torch_loss(rgb, mask, gt, gt_mask):
    """sum over the views of mean |rgb - gt| over the overlap + the reference's SSIM term, composed from torch operations (B, H, W, 3)"""
    ov = (mask != 0) & (gt_mask != 0)
    n = ov.reshape(ov.shape[0], -1).sum(1).clamp(min=1).float()
    l1 = ((rgb - gt).abs() * ov[..., None]).reshape(ov.shape[0], -1).sum(1) / (3.0 * n)
    x, y = (gt * ov[..., None]).permute(0, 3, 1, 2), (rgb * ov[..., None]).permute(0, 3, 1, 2)
    pool = lambda a: F.avg_pool2d(a, 3, 1, padding=1)
    mx, my = pool(x), pool(y)
    sx, sy, sxy = pool(x * x) - mx * mx, pool(y * y) - my * my, pool(x * y) - mx * my
    s = ((2 * mx * my + 1e-4) * (2 * sxy + 9e-4)) / ((mx * mx + my * my + 1e-4) * (sx + sy + 9e-4) + 1e-12)
    return l1.sum() + torch.clamp((1.0 - s) / 2.0, 0, 1).mean((1, 2, 3)).sum()


def main():
    import inspect
    from core.graph.deep_sdf_decoder import Decoder
    from core.sdfrenderer import SDFRenderer_color
    from distr import fixture
    import distr
    assert os.path.abspath(distr.__file__).startswith(TREE + os.sep), (distr.__file__, TREE)      # the package measured is the one named
    tag = 'tree %s' % TREE if ARGS.tree else 'this build'
    has_flag = 'color_decoder_grad' in inspect.signature(SDFRenderer_color.__init__).parameters

    def module(Ws, bs, latent, dims, last):
        d = Decoder(latent, dims, last_dim=last, norm_layers=(), latent_in=[4])
        d.load_state_dict({('lin%d.%s' % (l, n)): torch.from_numpy(a) for l, (W, b) in enumerate(zip(Ws, bs)) for n, a in (('weight', W), ('bias', b))})
        return d.cuda().eval()
    Ws, bs, latent = fixture.make_decoder_weights()
    Wc, bc, code = fixture.make_color_decoder_weights(color_size=CS)
    dims_c = [512] * 8
    dims_c[3] += CS
    dec, dec_c = module(Ws, bs, 256, [512] * 8, 1), module(Wc, bc, 256 + CS, dims_c, 3)
    for p in dec.parameters():
        p.requires_grad_(False)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()
    cams = [fixture.make_camera(30.0 + 40.0 * v, 20.0 - 5.0 * v, 1.6, 10.0) for v in range(B)]
    Rs, Ts = t(np.stack([c[0] for c in cams])), t(np.stack([c[1] for c in cams]))
    ren = SDFRenderer_color(dec, dec_c, fixture.make_intrinsic(SIZE, SIZE), img_hw=(SIZE, SIZE), march_step=STEPS, buffer_size=3)
    with torch.no_grad():
        _, _, rgb0, mask0, _ = ren.render_batch(t(code), t(latent), Rs, Ts)
    rs = np.random.RandomState(SIZE)
    gt = rgb0 + 0.1 * t(rs.standard_normal(tuple(rgb0.shape)))
    gt_mask = torch.roll(mask0, 3, dims=2)
    print('%s: %d views of %d x %d / %d steps, valid pixels per view %s' % (tag, B, SIZE, SIZE, STEPS, mask0.reshape(B, -1).sum(1).tolist()), flush=True)

    def step(loss_fn):
        for p in dec_c.parameters():
            p.grad = None
        cc, lat = t(code).requires_grad_(True), t(latent).requires_grad_(True)
        _, _, rgb, mask, _ = ren.render_batch(cc, lat, Rs, Ts)
        loss_fn(rgb, mask, gt, gt_mask).backward()
    med, raw = timed(lambda: step(torch_loss))
    print('%s: render_batch fwd + torch loss + bwd, flag off: %.2f ms  [%s]' % (tag, med, raw), flush=True)
    if not has_flag:
        return
    from core.utils.loss_utils import compute_loss_color_batch

    def fused_loss(rgb, mask, g, gm):
        l1, ssim, _ = compute_loss_color_batch(rgb, mask, g, gm, use_ssim=True)
        return l1.sum() + ssim.sum()
    ren.color_decoder_grad = True
    med, raw = timed(lambda: step(torch_loss))
    assert all(p.grad is not None for p in dec_c.parameters())
    print('%s: render_batch fwd + torch loss + bwd, flag on:  %.2f ms  [%s]' % (tag, med, raw), flush=True)
    med, raw = timed(lambda: step(fused_loss))
    print('%s: render_batch fwd + fused loss + bwd, flag on:  %.2f ms  [%s]' % (tag, med, raw), flush=True)
    for name, fn in (('fused', fused_loss), ('torch', torch_loss)):
        def alone():
            x = rgb0.clone().requires_grad_(True)
            fn(x, mask0, gt, gt_mask).backward()
        med, raw = timed(alone)
        print('%s: loss alone fwd + bwd, %s: %.3f ms  [%s]' % (tag, name, med, raw), flush=True)
    a = rgb0.clone().requires_grad_(True)
    b = rgb0.clone().requires_grad_(True)
    la, lb = fused_loss(a, mask0, gt, gt_mask), torch_loss(b, mask0, gt, gt_mask)
    la.backward()
    lb.backward()
    print('fused against torch: loss %.3e apart, gradient %.3e of its largest entry' % (abs(la.item() - lb.item()), ((a.grad - b.grad).abs().max() / b.grad.abs().max()).item()))


if __name__ == '__main__':
    main()
