"""Shared pieces of the tests of weight gradients through render (golden G33).

The CPU chain: the oracle's render of a scene, the sample list its backward builds from the upstream gradients of the scene's loss
(RenderState.samples), and tests/train_restatement.gradients in float64 over that list with the oracle's ReLU gates:
    dL/dtheta = sum over the list of coef * d f(x; theta) / d theta.
tests/gen_golden_render_weight_grad.py compares the chain with the reference when it chooses a case, tests/test_render_train_host.py pins
it to the golden, and tests/test_gpu_render_train.py takes its list (and float64 gradients on the GPU's gates) as expected values.
"""
import numpy as np

import helpers
import train_restatement as tr

ROWS = (0, 255, -1)
# case -> (keywords of the oracle's / binding's make_cfg, which outputs carry the loss)
CASES = {
    'pyr_d2n': (dict(marcher='pyramid_recursive', use_depth2normal=True, want_normal=True), 'render'),
    'rec_depth': (dict(marcher='recursive', want_normal=False), 'render_depth'),
    'wn': (dict(marcher='pyramid_recursive', use_depth2normal=True, want_normal=True), 'render'),
}


def cfg_kw(g, case):
    """make_cfg keywords of a G33 case (g: the loaded golden)."""
    kw = dict(CASES[case][0])
    kw.update(march_step=int(g['march_step']), buffer_size=int(g['buffer_size']))
    return kw


def wn_state_dict(g, Ws, bs):
    """The weight-norm decoder of the `wn` case as a numpy state dict: weight_v = the fixture's weights, weight_g as the reference's module
    held it (recorded in the golden)."""
    from distr import decoder_pack
    sd = decoder_pack.fixture_state_dict(Ws, bs, weight_norm=True)
    for l in range(8):
        sd['lin%d.weight_g' % l] = np.asarray(g['wn_weight_g%d' % l], np.float32).reshape(sd['lin%d.weight_g' % l].shape)
    return sd


def upstream(kind, H, W, seed, mask):
    """Upstream gradients of the seeded dense loss (helpers.loss_weights) as the backward takes them. 'render': L = sum(wd depth [mask]) +
    sum(wq min_sdf) + sum(wn normal); 'render_depth': L = sum(wd zdepth [mask]) + sum(wq min_sdf)."""
    wd, wq, wn = helpers.loss_weights(H, W, seed)
    m = np.asarray(mask).reshape(H, W).astype(np.float32)
    if kind == 'render':
        return dict(g_min_sdf=wq.reshape(-1), g_depth=(wd * m).reshape(-1), g_normal=wn.reshape(-1))
    return dict(g_zdepth=(wd * m).reshape(-1), g_min_sdf=wq.reshape(-1))


def oracle_gates(O, Ws, latent, pts):
    """The oracle's ReLU pattern at pts: eight boolean arrays (n, units of lin_l)."""
    return [O.layer_activations(latent, pts, l)[:, :Ws[l].shape[0]] > 0 for l in range(8)]


def oracle_list(O, orc, H, W, K, R, T, latent, seed, kind, **kw):
    """(render outputs, (pix, pts, coef)) of the oracle for the scene and its seeded loss."""
    out = O.render(orc.make_cfg(H, W, K, **kw), latent, R, T)
    return out, out['state'].samples(**upstream(kind, H, W, seed, out['mask']))


def chain_gradients(Ws, bs, latent, pts, coef, gates):
    """([g_W0..g_W8], [g_b0..g_b8], g_latent (1, C)) in float64: the sum over the list, every ReLU on `gates`."""
    import torch
    _, _, gW, gb, gc = tr.gradients(Ws, bs, latent, pts, [len(pts)], coef, None, [torch.as_tensor(np.asarray(g)) for g in gates])
    return [g.numpy() for g in gW], [g.numpy() for g in gb], gc.numpy()


def weight_norm_chain(sd, gW):
    """g_W of the folded weights W = v * (g / ||v||_row) carried on to (g_weight_g, g_weight_v) of lin0..lin7, in float64."""
    import torch
    gg, gv = [], []
    for l in range(8):
        v = torch.as_tensor(np.asarray(sd['lin%d.weight_v' % l]), dtype=torch.float64).clone().requires_grad_(True)
        g = torch.as_tensor(np.asarray(sd['lin%d.weight_g' % l]), dtype=torch.float64).clone().requires_grad_(True)
        ((v * (g.reshape(-1, 1) / v.norm(dim=1, keepdim=True))) * torch.as_tensor(np.asarray(gW[l]), dtype=torch.float64)).sum().backward()
        gg.append(g.grad.numpy().reshape(np.asarray(sd['lin%d.weight_g' % l]).shape))
        gv.append(v.grad.numpy())
    return gg, gv


def matrix_summary(name, M):
    """The recorded quantities of a large gradient matrix: row sums, column sums and the rows 0, 255 and last (lin3 has 253: 0, 252, 252)."""
    M = np.asarray(M)
    rows = [min(i, M.shape[0] - 1) if i >= 0 else M.shape[0] - 1 for i in ROWS]
    return {name + '_rowsum': M.sum(1), name + '_colsum': M.sum(0), name + '_rows': M[rows].copy()}


def recorded(gW, gb, g_weight_g=None, g_weight_v=None):
    """Every recorded quantity of the eighteen gradients: all biases, lin8.weight, and per large matrix its summary; a weight-norm decoder
    has weight_g of lin0..lin7 in full and the summaries of weight_v instead of those of the weights."""
    out = {'g_bias%d' % l: np.asarray(gb[l]) for l in range(9)}
    out['g_lin8_weight'] = np.asarray(gW[8])
    for l in range(8):
        if g_weight_v is None:
            out.update(matrix_summary('g_W%d' % l, gW[l]))
        else:
            out['g_weight_g%d' % l] = np.asarray(g_weight_g[l])
            out.update(matrix_summary('g_v%d' % l, g_weight_v[l]))
    return out


def residuals(got, g, case):
    """[(quantity, max |got - golden| / max |golden|, bar = max(1e-3, 2 x the golden's floor))] over EVERY recorded gradient quantity of the
    case (the keys '<case>_g_*' of the golden, none left out); `got` must have them all."""
    keys = sorted(k[len(case) + 1:] for k in g.keys() if k.startswith(case + '_g_'))
    assert keys and all(('%s_floor_%s' % (case, k)) in g for k in keys), keys
    out = []
    for k in keys:
        ref = np.asarray(g['%s_%s' % (case, k)], np.float64)
        a = np.asarray(got[k], np.float64).reshape(ref.shape)
        out.append((k, float(np.abs(a - ref).max() / np.abs(ref).max()), max(1e-3, 2.0 * float(g['%s_floor_%s' % (case, k)]))))
    return out
