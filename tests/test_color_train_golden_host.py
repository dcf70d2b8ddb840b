"""Golden G34 (tests/gen_golden_color_train.py: the reference's decode_color on 3 x 70 points under DeepSDF's specification, loss mean
|rgb - target|, evaluated by the reference itself) against the float64 restatement of the colour net, on the CPU. The float64 path has
no f32 chain error, so the bars are floor-dominated: values within max(2 x recorded floor, 1e-6), gradients within max(2 x floor, 1e-5)
of the quantity's largest entry; where a recorded floor exceeds the fixed part the floor rules, as for G32. In `train` the restatement
multiplies the relu outputs with this project's masks under the recorded seed (segment = index of the code pair, point = row inside the
segment) times float32(1 / (1 - p)) -- what the generator made the reference's F.dropout hand out."""
import os

import numpy as np
import pytest

from conftest import ROOT

GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'g34_color_train.npz')


@pytest.mark.parametrize('case', ['eval', 'train'])
def test_golden_g34_against_the_float64_restatement(case):
    import torch
    import color_train_restatement as cr
    import dropout_restatement as dr
    from distr import fixture
    g = np.load(GOLDEN)
    Ws, bs, _ = fixture.make_color_decoder_weights(color_size=256)
    assert str(g['weights_sha256']) == fixture.weights_sha256(Ws, bs)
    B, S = g['points'].shape[:2]
    assert (B, S) == (3, 70) and g['color_codes'].shape == (3, 256) and g['shape_codes'].shape == (3, 256)
    seed, p = int(g['seed']), float(g['p'])
    masks = None
    if case == 'train':
        masks = {l: dr.keep_list(seed, l, [S] * B, 253 if l == 3 else 512, dr.threshold(p)) for l in range(8)}
        for l in range(8):
            assert np.array_equal(masks[l], cr.g34_bits(g, 'train', 'keep', l)), l
    # weight norm as the generator loaded it: v = W, g = ||W||_row (f32), folded in float64 on the autograd graph
    v = [torch.tensor(W, dtype=torch.float64, requires_grad=True) for W in Ws[:8]]
    gn = [torch.from_numpy(W).norm(dim=1, keepdim=True).double().requires_grad_(True) for W in Ws[:8]]
    W8 = torch.tensor(Ws[8], dtype=torch.float64, requires_grad=True)
    b64 = cr.to64(bs, True)
    cc, sc = cr.to64([g['color_codes'], g['shape_codes']], True)
    W64 = [v[l] * (gn[l] / v[l].norm(dim=1, keepdim=True)) for l in range(8)] + [W8]
    y, pre = cr.forward(W64, b64, cc, sc, cr.to64([g['points'].reshape(-1, 3)])[0], [S] * B, masks=masks, scale=dr.scale(p))
    for l in range(8):
        diff = (pre[l] > 0).numpy() != cr.g34_bits(g, case, 'pos', l)
        assert not diff.any() or np.abs(pre[l].detach().numpy()[diff]).max() < 1e-5, l
        assert not (diff & ~cr.g34_bits(g, case, 'near', l)).any(), l
    loss = (y - cr.to64([g['target']])[0]).abs().mean()
    loss.backward()
    grads = {'lin8.weight': W8.grad}
    for l in range(9):
        grads['lin%d.bias' % l] = b64[l].grad
    for l in range(8):
        grads['lin%d.weight_g' % l], grads['lin%d.weight_v' % l] = gn[l].grad, v[l].grad
    q = cr.g34_quantities(y, loss, cc.grad, sc.grad, grads)
    cr.g34_check(g, case, q, 1e-6, 1e-5, 'float64 restatement')
