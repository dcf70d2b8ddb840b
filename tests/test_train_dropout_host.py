"""CPU-only checks of dropout on the layer-wise train path: the mask's definition (Philox4x32-10 known answers,
the library's host function against the numpy restatement, statistics of the definition), the parameter logic, the argument checks of
the C calls, and golden G32 (the reference's training forward under this project's masks) against the float64 restatement."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import ROOT

SIZES = [1, 64, 65, 0, 130, 63]
SEEDS = (1, 0x5EED0001, 0xA4093822299F31D0)
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'g32_train_forward.npz')


def _module(Ws, bs, weight_norm=False, **kw):
    import torch
    from core.graph.deep_sdf_decoder import Decoder
    from distr import decoder_pack
    dec = Decoder(decoder_pack.latent_size_of(Ws), [512] * 8, norm_layers=tuple(range(8)) if weight_norm else (), latent_in=[4], weight_norm=weight_norm, **kw)
    dec.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in decoder_pack.fixture_state_dict(Ws, bs, weight_norm=weight_norm).items()})
    return dec.eval()


def test_philox_known_answers():
    """The three Philox4x32-10 vectors of Random123's kat_vectors."""
    import dropout_restatement as dr
    F = 0xFFFFFFFF
    for counter, key, want in (((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
                               ((F, F, F, F), (F, F), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
                               ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))):
        got = tuple(int(x) for x in dr.philox4x32_10(counter, key))
        assert got == want, (counter, ['%08x' % x for x in got])
    assert dr.threshold(0.2) == 858993459 and dr.scale(0.2) == 1.25 and dr.threshold(0.5) == 1 << 31 and dr.scale(0.5) == 2.0


def test_library_keep_equals_the_restatement():
    """distr_train_dropout_keep is compiled from the round function the kernels call: this pins the device's mask without a GPU."""
    import dropout_restatement as dr
    from distr import binding
    binding.build_library()
    L = binding.lib()
    segments, units, points = [0, 1, 63, 64, 1 << 31], [0, 1, 252, 253, 511], np.arange(132)
    checked = 0
    for seed in (0,) + SEEDS:
        for p in (0.2, 0.5):
            T = dr.threshold(p)
            for layer in range(8):
                for g in segments:
                    want = dr.keep_at(seed, T, layer, g, points[:, None], np.asarray(units)[None, :])
                    got = np.array([[L.distr_train_dropout_keep(seed, T, layer, g, int(i), n) for n in units] for i in points])
                    assert np.array_equal(got, want.astype(got.dtype)), (seed, p, layer, g)
                    checked += got.size
    assert checked == 4 * 2 * 8 * 5 * 132 * 5


def test_train_dropout_params(fixture_decoder):
    from distr import functions
    Ws, bs, _ = fixture_decoder
    dec = _module(Ws, bs, dropout=list(range(8)), dropout_prob=0.2).train()
    assert functions.train_dropout_params(dec, 7) == (0xff, 858993459, 1.25)
    assert functions.train_dropout_params(dec, 7, segment_base=64) == (0xff, 858993459, 1.25)
    assert functions.train_dropout_params(dec.eval(), 7) is None
    half = _module(Ws, bs, dropout=[0, 3, 7], dropout_prob=0.5).train()
    assert functions.train_dropout_params(half, 0) == (0x89, 1 << 31, 2.0)
    assert functions.train_dropout_params(_module(Ws, bs, dropout=[0, 1], dropout_prob=0.0).train(), 1) is None
    assert functions.train_dropout_params(_module(Ws, bs, dropout=[], dropout_prob=0.2).train(), 1) is None
    assert functions.train_dropout_params(_module(Ws, bs, dropout=None, dropout_prob=0.2).train(), 1) is None
    with pytest.raises(ValueError, match='dropout_prob'):
        functions.train_dropout_params(_module(Ws, bs, dropout=[0], dropout_prob=1.0).train(), 1)
    with pytest.raises(ValueError, match='dropout_prob'):
        functions.train_dropout_params(_module(Ws, bs, dropout=[0], dropout_prob=-0.1).train(), 1)
    with pytest.raises(ValueError, match='layer 8'):
        functions.train_dropout_params(_module(Ws, bs, dropout=[0, 8], dropout_prob=0.2).train(), 1)
    with pytest.raises(ValueError, match='seed'):
        functions.train_dropout_params(dec.train(), -1)
    with pytest.raises(ValueError, match='segment_base'):
        functions.train_dropout_params(dec, 1, segment_base=-1)


def test_draw_dropout_seed_follows_the_cpu_generator():
    import torch
    from distr import functions
    torch.manual_seed(11)
    a = [functions.draw_dropout_seed() for _ in range(3)]
    torch.manual_seed(11)
    assert a == [functions.draw_dropout_seed() for _ in range(3)] and len(set(a)) == 3
    assert all(isinstance(s, int) and 0 <= s < 1 << 63 for s in a)
    g = torch.Generator().manual_seed(5)
    b = functions.draw_dropout_seed(g)
    assert b == functions.draw_dropout_seed(torch.Generator().manual_seed(5))


def test_decode_sdf_train_takes_a_seed(fixture_decoder):
    """On CPU tensors the call with a seed gets as far as the device check; latent_dropout in training mode stays refused."""
    import torch
    from core.utils import decoder_utils as du
    from distr import decoder_pack
    Ws, bs, _ = fixture_decoder
    lat, pts = torch.zeros(len(SIZES), 256), torch.zeros(sum(SIZES), 3)
    drop = _module(Ws, bs, dropout=list(range(8)), dropout_prob=0.2).train()
    with pytest.raises(RuntimeError, match='must be on the GPU'):
        du.decode_sdf_train(drop, lat, pts, counts=SIZES, dropout_seed=5)
    with pytest.raises(RuntimeError, match='must be on the GPU'):
        du.decode_sdf_train(drop.eval(), lat, pts, counts=SIZES, dropout_seed=5)
    with pytest.raises(decoder_pack.UnsupportedDecoder, match='training mode with dropout'):
        du.decode_sdf_train(drop.train(), lat, pts, counts=SIZES)
    ldrop = _module(Ws, bs, latent_dropout=True, dropout=[0], dropout_prob=0.2).train()
    with pytest.raises(decoder_pack.UnsupportedDecoder, match='latent_dropout'):
        du.decode_sdf_train(ldrop, lat, pts, counts=SIZES, dropout_seed=5)
    with pytest.raises(ValueError, match='dropout_prob'):
        du.decode_sdf_train(_module(Ws, bs, dropout=[0], dropout_prob=1.0).train(), lat, pts, counts=SIZES, dropout_seed=5)
    assert hasattr(drop, 'forward_train') and type(drop).forward is type(drop).inference


def test_c_calls_refuse_bad_dropout_structs():
    """The struct is checked before anything touches the device: a context made without one answers."""
    import train_abi
    from distr import binding
    binding.build_library()
    L = binding.lib()
    cnt = (C.c_int64 * 2)(5, 3)
    good = dict(layer_mask=0xff, threshold=858993459, scale=1.25, seed=1, segment_base=0)
    assert L.distr_train_forward_dropout(None, None, 2, cnt, None, 0, None, 0.1, None, None, 0, None, C.byref(binding.TrainDropout(**good))) == -1
    assert L.distr_train_backward_dropout(None, None, 2, cnt, None, 0, None, 0.1, None, None, None, None, C.byref(binding.TrainDropout(**good))) == -1
    assert C.sizeof(binding.TrainDropout) == 32
    h = C.c_void_p()
    L.distr_create_abi(C.byref(h), 0, binding.ABI_VERSION)          # (without a device this fails; the context still answers)
    assert h
    try:
        dummy = (C.c_float * 4)()
        tw = train_abi.train_weights([C.addressof(dummy)] * 18, 256)
        tg = train_abi.train_grads([C.addressof(dummy)] * 18)
        bad = [('struct_size', dict(good), 24), ('layer_mask', dict(good, layer_mask=0x100), None), ('scale', dict(good, scale=0.5), None),
               ('scale', dict(good, scale=float('nan')), None), ('scale', dict(good, scale=float('inf')), None),
               ('segment_base', dict(good, segment_base=-1), None)]
        for word, kw, size in bad:
            td = binding.TrainDropout(**kw)
            if size is not None:
                td.struct_size = size
            for rc in (L.distr_train_forward_dropout(h, C.byref(tw), 2, cnt, None, 0, None, 0.1, None, None, 0, None, C.byref(td)),
                       L.distr_train_backward_dropout(h, C.byref(tw), 2, cnt, None, 0, None, 0.1, None, C.byref(tg), None, None, C.byref(td))):
                err = L.distr_last_error(h).decode()
                assert rc == -1 and 'distr_train_dropout' in err and word in err, (word, kw, rc, err)
    finally:
        L.distr_destroy(h)


@pytest.mark.parametrize('p', [0.2, 0.5])
@pytest.mark.parametrize('seed', SEEDS)
def test_statistics_of_the_definition(seed, p):
    """Conditions on the definition, on the shapes of the GPU tests: the keep fraction overall and per layer, and no correlation between
    the masks of two layers, of adjacent units and of adjacent points."""
    import dropout_restatement as dr
    T = dr.threshold(p)
    masks = [dr.keep_list(seed, l, SIZES, 512, T).astype(np.float64) for l in range(8)]
    assert masks[0].shape == (sum(SIZES), 512)
    overall = np.mean([m.mean() for m in masks])
    per_layer = max(abs(m.mean() - (1 - p)) for m in masks)

    def corr(a, b):
        return abs(np.corrcoef(a.ravel(), b.ravel())[0, 1])
    c_layers = corr(masks[0], masks[1])
    c_units = corr(np.stack(masks)[:, :, :-1], np.stack(masks)[:, :, 1:])
    # adjacent points of one segment
    at, a, b = 0, [], []
    for n in SIZES:
        for m in masks:
            a.append(m[at:at + n][:-1].ravel())
            b.append(m[at:at + n][1:].ravel())
        at += n
    c_points = corr(np.concatenate(a), np.concatenate(b))
    print('seed %#x, p %.1f: keep fraction off by %.2e overall, %.2e per layer; |corr| layers %.2e units %.2e points %.2e'
          % (seed, p, abs(overall - (1 - p)), per_layer, c_layers, c_units, c_points))
    assert abs(overall - (1 - p)) <= 2e-3 and per_layer <= 5e-3
    assert c_layers <= 0.01 and c_units <= 0.01 and c_points <= 0.01


@pytest.mark.parametrize('case', ['eval', 'train'])
def test_golden_g32_against_the_float64_restatement(fixture_decoder, case):
    """The reference's training forward (G32) against train_restatement.forward in float64 on the fixture's weights: in `train` the gates
    are the recorded masks x the restatement's own ReLU x 1.25, fixed layer by layer. Values within max(2 x floor, 2e-6); the recorded
    masks are the restatement's under the recorded seed."""
    import torch
    import dropout_restatement as dr
    import train_restatement as tr
    from distr import fixture
    g = np.load(GOLDEN)
    Ws, bs, _ = fixture_decoder
    assert str(g['weights_sha256']) == fixture.weights_sha256(Ws, bs)
    B, S = g['sdf_data'].shape[:2]
    seed, p = int(g['seed']), float(g['p'])
    W64, b64 = tr.to64(Ws), tr.to64(bs)
    codes, data = tr.to64([g['codes']])[0], tr.to64([g['sdf_data'].reshape(-1, 4)])[0]
    gates = None
    if case == 'train':
        keeps = [dr.keep_list(seed, l, [S] * B, 509 - 256 if l == 3 else 512, dr.threshold(p)) for l in range(8)]
        for l in range(8):
            assert np.array_equal(keeps[l], dr.g32_bits(g, 'train', 'keep', l)), l
        gates = [torch.ones(B * S, k.shape[1], dtype=torch.float64) for k in keeps]
        for l in range(8):          # the gates of lin0..lin(l-1) are final: lin_l's pre-activation is, too
            _, pre = tr.forward(W64, b64, codes, data[:, :3], [S] * B, None, gates)
            gates[l] = torch.from_numpy(keeps[l].astype(np.float64) * dr.scale(p)) * (pre[l] > 0)
    y, pre = tr.forward(W64, b64, codes, data[:, :3], [S] * B, None, gates)
    for l in range(8):
        diff = (pre[l] > 0).numpy() != dr.g32_bits(g, case, 'pos', l)
        assert not diff.any() or pre[l].numpy()[diff].__abs__().max() < 1e-5, l
    lo, hi = tr.to64([g['min_vec'], g['max_vec']])
    pred = torch.minimum(torch.maximum(y, lo), hi)
    l1 = (pred - torch.minimum(torch.maximum(data[:, 3:4], lo), hi)).abs().squeeze(1)
    l2 = codes.pow(2).mean(1)
    for name, got in (('pred_sdf', pred), ('loss_l1', l1), ('loss_l2_size', l2)):
        want = g['%s_%s' % (case, name)]
        assert tuple(got.shape) == want.shape, name
        d = np.abs(got.numpy() - want).max()
        bar = max(2 * float(g['%s_floor_%s' % (case, name)]), 2e-6)
        print('G32 %s %s: |float64 - reference| <= %.3e (bar %.1e)' % (case, name, d, bar))
        assert d <= bar, (case, name, d)
