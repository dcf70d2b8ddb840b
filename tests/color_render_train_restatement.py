"""Shared pieces of the tests of the colour decoder's weight gradients through the colour render (golden G35).

The CPU chain of a case: the oracle's render of the scene (zdepth, mask, normal image); the colour stage restated in float64 torch -- the
valid pixels in row-major order, their rays and surface points x = M^T (c + d z) with z a constant, the colour decoder of
tests/color_train_restatement.py on them, with lights the shading term s = sum_m e_m ((R l_m) . n) -- the colour image, and the loss
l1 + ssim of tests/color_loss_restatement.py against the golden's target. From its backward:
  * the upstream of the colour image g_rgb, and from it THE DECOMPOSITION this project implements: the list (points, g_rgb * s) and
    color_train_restatement.gradients over it -> the eighteen weight gradients and the decoder's part of both code gradients;
  * the cameras' gradients through the points and the shading term, and g_normal, which the oracle's backward carries on to the shape
    code and the cameras (the geometry's part, as the fused render backward computes it).
tests/gen_golden_color_render_weight_grad.py compares the chain with the reference when it chooses a case, and
tests/test_color_render_train_host.py pins it to the golden.
"""
import numpy as np

import color_loss_restatement as clr
import color_train_restatement as ctr
import render_train_restatement as rt

H, W = 48, 40
K = np.array([[44.0, 0.0, W / 2.0], [0.0, 46.0, H / 2.0], [0.0, 0.0, 1.0]])
STEPS, BUF, CS = 24, 3, 32
M_POINT = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, -1.0], [0.0, 1.0, 0.0]])        # the default transform of make_cfg
# case -> (lit, weight-norm colour decoder)
CASES = {'unlit': (False, False), 'lit': (True, False), 'wn': (True, True)}
VALUES = ('rgb', 'l1', 'ssim')
SSIM_PAIRS = ((1, 1), (5, 7), (17, 19))


def oracle_cfg(orc):
    return orc.make_cfg(H, W, K, march_step=STEPS, buffer_size=BUF, marcher='recursive', use_depth2normal=False, want_normal=True)


def wn_state_dict(g, Wc, bc):
    """The weight-norm colour decoder of the `wn` case as a numpy state dict: weight_v = the fixture's weights, weight_g as the reference's
    module held it (recorded in the golden)."""
    from distr import decoder_pack
    sd = decoder_pack.fixture_state_dict(Wc, bc, weight_norm=True)
    for l in range(8):
        sd['lin%d.weight_g' % l] = np.asarray(g['wn_weight_g%d' % l], np.float32).reshape(sd['lin%d.weight_g' % l].shape)
    return sd


def chain(O, orc, case, Wc, bc, sd, latent, color_code, R, T, gt, gt_mask, lights, energies):
    """The CPU chain of a case -> (dict of every recorded quantity, the oracle's mask (H, W), number of list rows). Wc, bc: the colour
    decoder's plain weights; sd: the weight-norm state dict of the `wn` case (its folded weights are used) or None."""
    import torch
    from distr import decoder_pack
    lit = CASES[case][0]
    if sd is not None:
        Wc, bc = decoder_pack.effective_weights(sd)
    out = O.render(oracle_cfg(orc), latent, R, T)
    P = H * W
    mask = np.asarray(out['mask']).reshape(P) != 0
    idx = np.nonzero(mask)[0]
    N = len(idx)
    t64 = lambda a, g=False: torch.tensor(np.asarray(a, np.float64), dtype=torch.float64, requires_grad=g)
    Rt, Tt, nrm = t64(R, True), t64(T, True), t64(np.asarray(out['normal']).reshape(P, 3), True)
    z = t64(np.asarray(out['zdepth']).reshape(P)[idx])
    Kinv = np.linalg.inv(K).astype(np.float32).astype(np.float64)                  # (as make_cfg hands it to the kernels)
    h = t64(np.stack([idx % W, idx // W, np.ones(N)], 1) @ Kinv.T)
    r = h @ Rt                                                                     # R^T h
    d = r / (r.norm(dim=1, keepdim=True) + 1e-12)
    q = d * z[:, None] - (Tt @ Rt)                                                 # c = -R^T T
    x = q @ t64(M_POINT)                                                           # M^T q
    W64, b64 = ctr.to64(Wc, True), ctr.to64(bc, True)
    cc, sc = ctr.to64([color_code, latent], True)
    col, _ = ctr.forward(W64, b64, cc, sc, x, [N])
    s = torch.ones(N, dtype=torch.float64)
    if lit:
        s = torch.zeros(N, dtype=torch.float64)
        for Lm, em in zip(np.asarray(lights, np.float64), np.asarray(energies, np.float64)):
            u = t64(Lm)[None] - q
            l = u / u.norm(dim=1, keepdim=True)
            s = s + em * ((l @ Rt.t()) * nrm[idx]).sum(1)
    img = torch.zeros(P, 3, dtype=torch.float64).index_copy(0, torch.as_tensor(idx), col * s[:, None]).reshape(H, W, 3)
    img.retain_grad()
    l1, ssim = clr.torch_color_loss(img, torch.as_tensor(mask.reshape(H, W)), t64(gt), torch.as_tensor(np.asarray(gt_mask).reshape(H, W) != 0))
    (l1 + ssim).backward()
    # the decomposition: the list and its upstream, the train path's float64 restatement over it
    up = img.grad.reshape(P, 3)[idx].numpy() * s.detach().numpy()[:, None]
    _, _, gW, gb, g_cc, g_sc = ctr.gradients(Wc, bc, color_code, latent, x.detach().numpy(), [N], up)
    gW, gb = [g.numpy() for g in gW], [g.numpy() for g in gb]
    for a, b in zip(gW + gb + [g_cc.numpy(), g_sc.numpy()], [t.grad.numpy() for t in W64 + b64 + [cc, sc]]):
        assert np.abs(a - b).max() <= 1e-9 * max(np.abs(b).max(), 1e-300), 'the decomposition is not the graph\'s gradient'
    g_lat, g_R, g_T = g_sc.numpy().copy(), Rt.grad.numpy().copy(), Tt.grad.numpy().copy()
    if lit:                                                                        # the normal image's gradient, through the render
        o_lat, o_R, o_T, _ = out['state'].backward(g_normal=nrm.grad.numpy().astype(np.float32).reshape(-1))
        g_lat, g_R, g_T = g_lat + o_lat, g_R + o_R, g_T + o_T
    got = rt.recorded(gW, gb, *(rt.weight_norm_chain(sd, gW) if sd is not None else ()))
    got.update(g_color_code=g_cc.numpy(), g_latent=g_lat, g_R=g_R, g_T=g_T, rgb=img.detach().numpy(), l1=np.float64(l1.item()), ssim=np.float64(ssim.item()))
    return got, mask.reshape(H, W), N


def residuals(got, g, case):
    """[(quantity, residual, bar = max(1e-3, 2 x the golden's floor))] over EVERY recorded quantity of the case: the gradients relative to
    the largest entry of the golden's quantity (render_train_restatement.residuals), the values rgb, l1, ssim absolute."""
    out = rt.residuals(got, g, case)
    for k in VALUES:
        ref = np.asarray(g['%s_%s' % (case, k)], np.float64)
        out.append((k, float(np.abs(np.asarray(got[k], np.float64).reshape(ref.shape) - ref).max()), max(1e-3, 2.0 * float(g['%s_floor_%s' % (case, k)]))))
    return out
