"""CPU-only checks of weight gradients through render: the decomposition dL/dtheta = sum over the backward's sample
list of coef * d f / d theta against the reference (golden G33), the plan that cuts the list into train calls, and the new part of the C
ABI (include/distr_render_train.h) against the binding and the library."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

import render_train_restatement as rt

G33 = os.path.join(GOLDEN, 'g33_render_weight_grad.npz')


@pytest.fixture(scope='module')
def g33():
    return dict(np.load(G33))


# ------------------------------------------------------------------------------------------------ the decomposition against the reference
def test_g33_is_complete_and_small(g33, fixture_decoder):
    from distr import fixture
    assert os.path.getsize(G33) < 400 << 10                                        # (G32: 0.5 MB)
    assert str(g33['weights_sha256']) == fixture.weights_sha256(*fixture_decoder[:2])
    assert sorted(str(c) for c in g33['case_names']) == sorted(rt.CASES)
    assert int(g33['noise_draws']) >= 3
    for case in rt.CASES:
        names = [k[len(case) + 1:] for k in g33 if k.startswith(case + '_g_')]
        want = ['g_latent', 'g_R', 'g_T', 'g_lin8_weight'] + ['g_bias%d' % l for l in range(9)]
        mats = ['g_v%d' % l for l in range(8)] if case == 'wn' else ['g_W%d' % l for l in range(8)]
        want += [m + s for m in mats for s in ('_rowsum', '_colsum', '_rows')] + (['g_weight_g%d' % l for l in range(8)] if case == 'wn' else [])
        assert sorted(names) == sorted(want), case
        for k in names:
            assert np.abs(g33['%s_%s' % (case, k)]).max() > 0 and 0 <= float(g33['%s_floor_%s' % (case, k)]) < 0.1, (case, k)
        assert int(g33[case + '_num_samples']) > 1000 and g33[case + '_mask'].sum() > 100


@pytest.mark.parametrize('case', sorted(rt.CASES))
def test_cpu_chain_matches_the_reference(g33, orc, fixture_decoder, case):
    """The oracle's sample list + float64 gradients on the oracle's gates against the reference's own backward with the decoder's
    parameters requiring grad: every recorded quantity inside max(1e-3, 2 x its floor). This pins the decomposition the GPU path
    implements to the reference; g_R / g_T are the oracle's backward of the same upstream gradients."""
    from distr import decoder_pack
    Ws, bs, latent = fixture_decoder
    assert np.array_equal(latent, g33['latent'])
    sd = None
    if case == 'wn':
        sd = rt.wn_state_dict(g33, Ws, bs)
        Ws, bs = decoder_pack.effective_weights(sd)
    H, W, seed, kind = int(g33['H']), int(g33['W']), int(g33['loss_seed']), rt.CASES[case][1]
    O = orc.Oracle(Ws, bs)
    out, (pix, pts, coef) = rt.oracle_list(O, orc, H, W, g33['K'], g33['R'], g33['T'], latent, seed, kind, **rt.cfg_kw(g33, case))
    assert len(pix) == int(g33[case + '_num_samples'])
    assert int((out['mask'].reshape(-1) != g33[case + '_mask'].reshape(-1)).sum()) <= 1
    _, gR, gT, _ = out['state'].backward(**rt.upstream(kind, H, W, seed, out['mask']))
    gW, gb, gc = rt.chain_gradients(Ws, bs, latent, pts, coef, rt.oracle_gates(O, Ws, latent, pts))
    got = rt.recorded(gW, gb, *(rt.weight_norm_chain(sd, gW) if sd is not None else ()))
    got.update(g_latent=gc, g_R=gR, g_T=gT)
    res = rt.residuals(got, g33, case)
    print(case, '%d samples;' % len(pix), ', '.join('%s %.1e' % (k, r) for k, r, _ in res))
    bad = [(k, r, bar) for k, r, bar in res if not r <= bar]
    assert not bad, (case, bad)


# ------------------------------------------------------------------------------------------------ the plan of the train calls
def _check_plan(counts, limit):
    from distr import binding, functions
    plan = functions.render_train_chunks(counts, limit)
    assert plan == functions.render_train_chunks(list(counts), limit)            # a function of its arguments alone
    seen = [[] for _ in counts]
    last = (-1, -1)
    for piece in plan:
        assert 1 <= len(piece) <= binding.MAX_SEGMENTS
        assert functions.train_plan_bytes([n for _, _, n in piece]) <= limit
        for v, a, n in piece:
            assert n > 0 and a % 64 == 0 and a + n <= counts[v]
            assert (v, a) > last                                                  # view order, then row order
            last = (v, a)
            seen[v].append((a, n))
    for v, c in enumerate(counts):                                                # every row exactly once, no gap
        at = 0
        for a, n in seen[v]:
            assert a == at
            at += n
        assert at == c
    return plan


def test_chunks_cover_every_point_once():
    from distr import functions
    big = 1 << 40
    assert functions.render_train_chunks([], big) == [] and functions.render_train_chunks([0, 0, 0], big) == []
    assert _check_plan([2708], big) == [[(0, 0, 2708)]]
    assert _check_plan([5, 0, 64, 0, 65], big) == [[(0, 0, 5), (2, 0, 64), (4, 0, 65)]]        # empty views get no segment
    # one view longer than the limit: cut at multiples of 64 rows from its start, the remainder last
    lim = functions.train_plan_bytes([256])
    plan = _check_plan([1000], lim)
    assert [p[0][1:] for p in plan] == [(0, 256), (256, 256), (512, 256), (768, 232)]
    # a cut inside a view while the piece already holds other views; later views start new pieces
    plan = _check_plan([100, 0, 300, 64, 7], functions.train_plan_bytes([128, 128]))
    assert len(plan) >= 3 and any(len(p) > 1 for p in plan) and any(a > 0 for p in plan for _, a, _ in p)
    # more than 64 views with rows: at most 64 segments per piece
    plan = _check_plan([3] * 150, big)
    assert [len(p) for p in plan] == [64, 64, 22]
    rs = np.random.RandomState(33)
    for _ in range(20):
        counts = [int(c) for c in rs.choice([0, 1, 63, 64, 65, 200, 1000, 5000], rs.randint(1, 9))]
        _check_plan(counts, functions.train_plan_bytes([int(rs.choice([64, 128, 640, 4096]))] * int(rs.randint(1, 3))))
    with pytest.raises(ValueError):
        functions.render_train_chunks([10], functions.train_plan_bytes([64]) - 1)
    with pytest.raises(ValueError):
        functions.render_train_chunks([10, -1], big)


def test_train_plan_bytes_mirrors_the_library():
    from distr import binding, functions
    binding.build_library()
    L = binding.lib()
    for counts in ([1], [64], [65, 0, 3], [2708], [0], [16385] * 5, [100000, 5, 7000], [3] * 64):
        cnt = (C.c_int64 * len(counts))(*counts)
        for Cn in (256, 64, 300):
            assert L.distr_train_workspace_bytes(Cn, len(counts), cnt) == functions.train_plan_bytes(counts), (counts, Cn)


# ------------------------------------------------------------------------------------------------ header, binding, library
def test_render_train_abi_declared_exported_and_checked():
    from distr import binding
    hdr = open(os.path.join(ROOT, 'include', 'distr_render_train.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    assert set(re.findall(r'\b(distr_[a-z0-9_]+)\s*\(', hdr)) == set(binding.RENDER_TRAIN_EXPORTS)
    top = open(os.path.join(ROOT, 'include', 'distr.h')).read()
    assert '#include "distr_render_train.h"' in top and 'distr_render_train.h' in binding.HEADERS
    assert 'DISTR_ABI_VERSION 6u' in top and binding.ABI_VERSION == 6
    binding.build_library()
    L = binding.lib()
    for name in binding.RENDER_TRAIN_EXPORTS:
        assert hasattr(L, name), name
    assert int(L.distr_abi_version()) == 6


def test_export_refusals_without_a_device():
    """The checks of distr_render_samples_export_batch are host code: a context created without a device still answers them (as
    test_depth_samples_host.py does for its entry points)."""
    from distr import binding
    binding.build_library()
    L = binding.lib()
    K = np.array([[44., 0, 20], [0, 46., 24], [0, 0, 1]])
    cfg = binding.make_cfg((48, 40), K, march_step=24, buffer_size=3, marcher='recursive', want_normal=False)
    cap = L.distr_render_max_samples(C.byref(cfg))
    assert cap == 48 * 40 * 3 + 1
    band = binding.make_cfg((48, 40), K, march_step=24, buffer_size=2, marcher='recursive', want_normal=False, band=(8, 16))
    assert L.distr_render_max_samples(C.byref(band)) == 16 * 40 * 2 + 1
    bad = cfg.clone()
    bad.buffer_size = 0
    assert L.distr_render_max_samples(C.byref(bad)) == 0 and L.distr_render_max_samples(None) == 0
    bad = cfg.clone()
    bad.struct_size -= 4
    assert L.distr_render_max_samples(C.byref(bad)) == 0
    split = cfg.clone()
    split.arith = binding.ARITH['bf16x6']                                    # (no context to ask for a decoder: the cfg alone is judged)
    assert L.distr_render_max_samples(C.byref(split)) == cap

    h = C.c_void_p()
    L.distr_create_abi(C.byref(h), 0, binding.ABI_VERSION)                   # (fails for lack of a device; the context still answers)
    fwd, bwd = C.c_size_t(), C.c_size_t()
    assert L.distr_workspace_bytes(h, C.byref(cfg), C.byref(fwd), C.byref(bwd)) == 0
    p = C.c_void_p(4096)                                                     # never dereferenced: every call below is refused before a launch
    INVALID, WORKSPACE = -1, -4

    def call(c=cfg, nviews=1, ws=p, ws_bytes=None, wb=p, wb_bytes=None, xyz=p, coef=p, src=None, cap_=cap, counts=p):
        return L.distr_render_samples_export_batch(h, C.byref(c), nviews, ws, fwd.value * nviews if ws_bytes is None else ws_bytes, wb,
                                                   bwd.value * nviews if wb_bytes is None else wb_bytes, xyz, coef, src, cap_, counts, None)
    assert L.distr_render_samples_export_batch(None, C.byref(cfg), 1, p, fwd.value, p, bwd.value, p, p, None, cap, p, None) == INVALID
    for kw in (dict(ws=None), dict(wb=None), dict(xyz=None), dict(coef=None), dict(counts=None)):
        assert call(**kw) == INVALID and b'null' in L.distr_last_error(h), kw
    off = cfg.clone()
    off.save_for_backward = 0
    assert call(c=off) == INVALID and b'save_for_backward' in L.distr_last_error(h)
    assert call(cap_=cap - 1) == INVALID and b'cap' in L.distr_last_error(h)
    assert call(nviews=0) == INVALID and call(nviews=65) == INVALID and b'nviews' in L.distr_last_error(h)
    assert call(c=bad) == INVALID and b'struct_size' in L.distr_last_error(h)
    assert call(ws_bytes=fwd.value - 1) == WORKSPACE and b'forward workspace' in L.distr_last_error(h)
    assert call(wb_bytes=bwd.value - 1) == WORKSPACE and b'backward workspace' in L.distr_last_error(h)
    assert call(nviews=2, wb_bytes=2 * bwd.value - 1) == WORKSPACE
    L.distr_destroy(h)


def test_refusals_of_the_python_layer():
    """check_render_weights: what weight gradients through render are not defined for, each with its reason."""
    from distr import binding, functions
    K = np.array([[44., 0, 20], [0, 46., 24], [0, 0, 1]])
    w = [None] * 18
    ok = binding.make_cfg((48, 40), K, march_step=24, buffer_size=3, use_depth2normal=True)
    functions.check_render_weights(ok, w)
    functions.check_render_weights(binding.make_cfg((48, 40), K, march_step=24, buffer_size=3, want_normal=False), w)
    agn = binding.make_cfg((48, 40), K, march_step=24, buffer_size=3, use_depth2normal=False)
    functions.check_render_weights(agn, w, normals_detached=True)
    with pytest.raises(NotImplementedError, match='normals from depth'):
        functions.check_render_weights(agn, w)
    with pytest.raises(NotImplementedError, match="arith='f32' only"):
        functions.check_render_weights(binding.make_cfg((48, 40), K, march_step=24, buffer_size=3, use_depth2normal=True, arith='bf16x6'), w)
    with pytest.raises(NotImplementedError, match='row bands'):
        functions.check_render_weights(binding.make_cfg((48, 40), K, march_step=24, buffer_size=3, use_depth2normal=True, band=(8, 16)), w)
    with pytest.raises(NotImplementedError, match='normal_decoder_grad'):
        functions.check_render_weights(ok, w, normal_decoder_grad=True)
    with pytest.raises(ValueError, match='18 tensors'):
        functions.check_render_weights(ok, w[:17])
