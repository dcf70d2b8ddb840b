"""Renders in which the step kernel's 32-ray role does the work, compacted (DISTR_COMPACT32=1, the default) against dense (0) in a second
context: a ray's values depend neither on the size of its tile nor on which of the tile's hidden units the k-loop walks, so every output
and gradient must be BYTE-identical, and both agree with the oracle at the bars of tests/test_gpu_live_order.py.

Scene A: 64 x 64 / 20 steps with DISTR_TAIL16_THRESHOLD=64 and DISTR_HYBRID_THRESHOLD=8192 -- 4096 rays at most, so a step never has a
64-ray round and every step with more than 64 live rays runs on 32-ray tiles alone (atomic append behind them).
Scene B: the 136 x 144 scene of test_gpu_live_order.py with DISTR_TAIL16_THRESHOLD=64 -- step 0 has a round of 64-ray tiles and a 32-ray
remainder, so the step is ORDERED and slot_append<32> runs behind a compacted tile.
The 32-ray tiles' k-step counter (render_stats(ksteps=True)['ksteps32'], per full-resolution step): tiles = ceil(rays / 32), and
0 < executed < dense with the knob on, executed = dense with it off."""
import numpy as np
import pytest

from test_gpu_live_order import GRADS, OUTS, _camera, _diff, _engine, _render, _view

pytestmark = pytest.mark.gpu

ENV_A = dict(DISTR_TAIL16_THRESHOLD=64, DISTR_HYBRID_THRESHOLD=8192)
ENV_B = dict(DISTR_TAIL16_THRESHOLD=64)
KW_A = {'pyramid_recursive': dict(march_step=20, buffer_size=3, marcher='pyramid_recursive', use_depth2normal=True),
        'recursive': dict(march_step=20, buffer_size=3, marcher='recursive', use_depth2normal=True)}
KW_B = dict(march_step=16, buffer_size=3, marcher='pyramid_recursive', use_depth2normal=True)
MARCHERS = sorted(KW_A)
T16 = 64


def _pair(fixture_decoder, env, **more):
    """(compacted, dense) 32-ray role: two contexts that differ in DISTR_COMPACT32 only."""
    return tuple(_engine(fixture_decoder, DISTR_COMPACT32=v, **env, **more) for v in (1, 0))


def _pad(c, g):
    return (c + g - 1) // g * g


def _steps32(eng, r):
    """Per full-resolution step that ran as a k_step launch: (live rays, the 32-ray tiles' counter)."""
    node = r['node']
    st = eng.ctx.render_stats(node.cfg, node.ws, ksteps=True)
    ks = st['ksteps32']
    counts = eng.ctx.live_counts(node.cfg, node.ws)[-len(ks):]
    assert len(counts) == len(ks) > 0
    n = min(len(ks), st['tail_from'])        # (steps from tail_from on share the persistent tail launch: 16-ray tiles only)
    return list(zip(counts[:n], ks[:n]))


@pytest.fixture(scope='module')
def engines_a(fixture_decoder):
    return _pair(fixture_decoder, ENV_A)


@pytest.fixture(scope='module')
def renders_a(engines_a, fixture_decoder):
    """Scene A in both modes, per marcher: rendered once, shared, never modified."""
    return {m: tuple(_render(e, fixture_decoder[2], 64, 64, [_camera()], KW_A[m]) for e in engines_a) for m in MARCHERS}


@pytest.mark.parametrize('marcher', MARCHERS)
def test_scene_a_bytes_and_oracle(renders_a, cpu_oracle, orc, fixture_decoder, marcher):
    import helpers
    from distr import fixture
    on, off = renders_a[marcher]
    assert on['mask'].sum() > 100
    assert _diff(on, off) == []
    R, T = _camera()
    ref = helpers.oracle_render(cpu_oracle, orc, 64, 64, fixture.make_intrinsic(64, 64), R, T, fixture_decoder[2], **KW_A[marcher])
    res = helpers.compare(_view(on, 0, 64, 64), ref, 64, 64, tol_depth=1e-6, tol_grad=1e-4, normal_p99=1e-5, max_flip_frac=0.0)
    print('residuals against the oracle:', res)


@pytest.mark.parametrize('marcher', MARCHERS)
def test_scene_a_counter(engines_a, renders_a, marcher):
    """Every step above 64 live rays: ceil(rays / 32) tiles of 32 rays, none elsewhere; the compacted tiles executed fewer k-steps than as
    many dense ones (and not none), the dense ones exactly 768 each."""
    per_mode = [_steps32(e, r) for e, r in zip(engines_a, renders_a[marcher])]
    print('rays, (tiles, executed, dense) per step:', per_mode[0])
    assert [c for c, _ in per_mode[0]] == [c for c, _ in per_mode[1]]
    big = [i for i, (c, _) in enumerate(per_mode[0]) if _pad(c, 16) > T16]
    assert len(big) >= 3, per_mode[0]
    for mode, steps in enumerate(per_mode):
        for i, (c, (tiles, done, dense)) in enumerate(steps):
            if i in big:
                assert tiles == (c + 31) // 32 and dense == 768 * tiles, (i, c, tiles, dense)
                assert (0 < done < dense) if mode == 0 else (done == dense), (mode, i, done, dense)
            else:
                assert (tiles, done, dense) == (0, 0, 0), (i, c, tiles)
    # the 64-ray counter does not see these tiles
    node = renders_a[marcher][0]['node']
    ks64 = engines_a[0].ctx.render_stats(node.cfg, node.ws, ksteps=True)['ksteps']
    assert all(k[0] == 0 for k in ks64[-len(per_mode[0]):]), ks64


def test_scene_a_without_saved_masks(fixture_decoder, renders_a):
    """DISTR_SAVE_MASKS=0 (the variants of the step kernel that keep no masks; the backward recomputes the decoder): the same bytes."""
    m = 'pyramid_recursive'
    on, off = (_render(e, fixture_decoder[2], 64, 64, [_camera()], KW_A[m]) for e in _pair(fixture_decoder, ENV_A, DISTR_SAVE_MASKS=0))
    assert _diff(on, off) == []
    assert _diff(on, renders_a[m][0], OUTS) == []


def test_scene_b_ordered_step_with_a_32_ray_remainder(fixture_decoder, cpu_oracle, orc):
    import helpers
    from distr import fixture
    from test_gpu_live_order import H, W, _round_step
    engines = _pair(fixture_decoder, ENV_B)
    on, off = (_render(e, fixture_decoder[2], H, W, [_camera()], KW_B) for e in engines)
    assert _diff(on, off) == []
    steps = _steps32(engines[0], on)
    print('rays, (tiles, executed, dense) per step:', steps)
    c0, (tiles, done, dense) = steps[0]
    # step 0: a round of 256 x 64 rays on the 64-ray role (so the step keeps its list in order) and the rest on 32-ray tiles
    assert _round_step(c0, t16=T16) and c0 > 16384 + T16 and tiles == (c0 - 16384 + 31) // 32 and 0 < done < dense, steps[0]
    R, T = _camera()
    ref = helpers.oracle_render(cpu_oracle, orc, H, W, fixture.make_intrinsic(H, W), R, T, fixture_decoder[2], **KW_B)
    res = helpers.compare(_view(on, 0, H, W), ref, H, W, tol_depth=1e-6, tol_grad=1e-4, normal_p99=1e-5, max_flip_frac=0.0)
    print('residuals against the oracle:', res)


def test_batch_of_two_views(engines_a, fixture_decoder):
    """Two cameras in one launch sequence on scene A's thresholds: the 32-ray role walks the virtual concatenation of the views' lists;
    each view equals its stand-alone render."""
    import helpers
    kw = KW_A['pyramid_recursive']
    cams = [helpers.bench_camera(0), helpers.bench_camera(3)]
    on, off = (_render(e, fixture_decoder[2], 64, 64, cams, kw) for e in engines_a)
    assert _diff(on, off) == []
    ks = engines_a[0].ctx.render_stats(on['node'].cfg, on['node'].ws, ksteps=True)['ksteps32']
    assert sum(k[0] for k in ks) > 0 and all(0 < k[1] < k[2] for k in ks if k[0]), ks
    for v, cam in enumerate(cams):
        alone = _render(engines_a[0], fixture_decoder[2], 64, 64, [cam], kw)
        bad = [k for k in OUTS + GRADS if np.asarray(on[k][v]).tobytes() != np.asarray(alone[k][0]).tobytes()]
        assert bad == [], (v, bad)
