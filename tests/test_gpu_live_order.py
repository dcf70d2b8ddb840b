"""The ordered live list of the full-resolution march (DISTR_LIVE_ORDER, DESIGN section 3, include/distr_live_order.h): a step whose 64-ray
role has work leaves the rays that stay live in the order of the list it read (slots per tile + k_live_pack) instead of in the completion
order of its tiles, and the setup kernels enumerate pixels in 16 x 16 blocks. A ray's values depend neither on its place in a tile nor on
its tile's company, so every output and gradient must be BYTE-identical to the atomic append (knob 0) in a second context.

Scene: fixture F1 from the fixture's camera at distance 1.6; the unit sphere (angular radius 38.7 deg) covers the whole image (half field
of view 26.6 deg), so every pixel is a ray: 136 x 144 = 19 584 rays = one round of 256 x 64 and a remainder in step 0, the 32- and
16-ray regimes later.

Two statements of the issue cannot be tested as written, and are tested in the nearest form the library allows:
  * a row band with row0 = 3: check_cfg refuses it (bands start on a multiple of 4: the pyramid's coarsest scale). Tested: that refusal, and
    the band [4, 128) -- row0 and rows are no multiples of 8, so the band's blocks are not the image's.
  * "run to run identical" lists: the list that enters step 0 is appended per workgroup of k_fine_init, atomically across workgroups (the
    issue allows that), so whole lists differ between runs by the order of 256-ray chunks. Tested: in each of two runs the list a step left
    is exactly the list it READ (same run, distr_debug_live_list returns both) with the non-survivors struck out, and the two runs' lists
    hold the same rays."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

H, W = 136, 144
T16, T32 = 4096, 8192              # the library's defaults (DISTR_TAIL16_THRESHOLD, DISTR_HYBRID_THRESHOLD)
OUTS = ('zdepth', 'mask', 'min_sdf', 'depth', 'normal')
GRADS = ('g_latent', 'g_R', 'g_T')
KW = {'pyramid_recursive': dict(march_step=16, buffer_size=3, marcher='pyramid_recursive', use_depth2normal=True),
      'recursive': dict(march_step=16, buffer_size=3, marcher='recursive', use_depth2normal=True)}
MARCHERS = sorted(KW)


def _engine(fixture_decoder, **env):
    """A context of its own with the knobs set (they are read at distr_create)."""
    from distr import functions
    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        return functions.engine_from_weights(fixture_decoder[0], fixture_decoder[1], 0)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope='module')
def engines(fixture_decoder):
    return _engine(fixture_decoder, DISTR_LIVE_ORDER=1), _engine(fixture_decoder, DISTR_LIVE_ORDER=0)


@pytest.fixture(scope='module')
def strips(fixture_decoder):
    """The schedule before the ordered list: pixels in strips of 256, atomic append."""
    return _engine(fixture_decoder, DISTR_LIVE_ORDER=0, DISTR_RAY_BLOCKS=0)


def _camera():
    from distr import fixture
    return fixture.make_camera(30, 20, 1.6, 10)


def _render(eng, latent, h, w, cams, kw, band=None):
    """B views (cams = [(R, T)]) through render_batch_call, the loss of helpers.hip_render per view, backward. -> dict of numpy arrays
    ([B, ...]) + 'node' (the autograd node: cfg, ws, view_bytes) + 'inputs'."""
    import torch
    import helpers
    from distr import binding, fixture, functions
    dev = eng.device
    B = len(cams)
    cfg = binding.make_cfg((h, w), fixture.make_intrinsic(h, w), band=band, **kw)
    rows = cfg.band_rows
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev).requires_grad_(True)
    lat, Rs, Ts = t(np.repeat(np.asarray(latent, np.float32).reshape(1, -1), B, 0)), t(np.stack([c[0] for c in cams])), t(np.stack([c[1] for c in cams]))
    z, mask, q, depth, normal = functions.render_batch_call(eng, cfg, lat, Rs, Ts)
    node = q.grad_fn
    wd, wq, wn = (torch.from_numpy(a).to(dev) for a in helpers.loss_weights(rows, w, 5))
    L = 0
    for v in range(B):
        mb = mask[v].reshape(rows, w).bool()
        L = L + (depth[v].reshape(rows, w) * wd)[mb].sum() + (q[v].reshape(rows, w) * wq).sum() + (normal[v].reshape(rows, w, 3) * wn).sum()
    L.backward()
    torch.cuda.synchronize()
    n = lambda x: x.detach().cpu().numpy()
    return dict(zdepth=n(z), mask=n(mask), min_sdf=n(q), depth=n(depth), normal=n(normal), g_latent=n(lat.grad), g_R=n(Rs.grad), g_T=n(Ts.grad),
                node=node, inputs=(lat, Rs, Ts), cfg=cfg)


def _diff(a, b, keys=OUTS + GRADS):
    return [k for k in keys if np.asarray(a[k]).tobytes() != np.asarray(b[k]).tobytes()]


def _view(a, v, rows, w):
    """View v of a batch result in the shapes helpers.compare expects."""
    return dict(zdepth=a['zdepth'][v], mask=a['mask'][v], min_sdf=a['min_sdf'][v], depth=a['depth'][v].reshape(rows, w),
                normal=a['normal'][v].reshape(rows, w, 3), g_latent=a['g_latent'][v], g_R=a['g_R'][v].reshape(3, 3), g_T=a['g_T'][v])


def _pad(c, g):
    return (c + g - 1) // g * g


def _round_step(c, t16=T16, t32=T32):
    """Restatement of step_ordered for one view: the 64-ray role of a step with c live rays has work (whole rounds or a big remainder)."""
    if _pad(c, 16) <= t16:
        return False
    n64 = _pad(c, 64)
    full = n64 // 16384 * 16384
    return full > 0 or n64 - full > t32 + t16


def _fine_counts(eng, r, kw):
    """Live rays entering every full-resolution step, and the k-step counters of those steps (the last entries of the launch lists)."""
    node = r['node']
    fine = kw['march_step'] - (6 if kw['marcher'] == 'pyramid_recursive' else 0)
    counts = eng.ctx.live_counts(node.cfg, node.ws)
    ks = eng.ctx.render_stats(node.cfg, node.ws, ksteps=True)['ksteps']
    assert len(counts) == len(ks) == kw['march_step']
    return counts[-fine:], ks[-fine:]


@pytest.fixture(scope='module')
def main_renders(engines, fixture_decoder):
    """The 136 x 144 scene in both modes, per marcher: rendered once, shared, never modified."""
    latent = fixture_decoder[2]
    return {m: tuple(_render(e, latent, H, W, [_camera()], KW[m]) for e in engines) for m in MARCHERS}


@pytest.mark.parametrize('marcher', MARCHERS)
def test_outputs_and_gradients_bytewise(engines, main_renders, cpu_oracle, orc, fixture_decoder, marcher):
    import helpers
    from distr import fixture
    on, off = main_renders[marcher]
    assert _diff(on, off) == []
    counts, ks = _fine_counts(engines[0], on, KW[marcher])
    print('live rays per step:', counts)
    # the scene is what the docstring says: every pixel a ray, a full round + remainder in step 0, the smaller regimes later
    assert engines[0].ctx.render_stats(on['node'].cfg, on['node'].ws)['num_in_sphere'] == H * W
    assert counts[0] > 16384 and _round_step(counts[0]) and not _round_step(counts[-1])
    assert any(T16 < _pad(c, 16) and not _round_step(c) for c in counts) and any(0 < _pad(c, 16) <= T16 for c in counts), counts
    R, T = _camera()
    ref = helpers.oracle_render(cpu_oracle, orc, H, W, fixture.make_intrinsic(H, W), R, T, fixture_decoder[2], **KW[marcher])
    res = helpers.compare(_view(on, 0, H, W), ref, H, W, tol_depth=1e-6, tol_grad=1e-4, normal_p99=1e-5, max_flip_frac=0.0)
    print('residuals against the oracle:', res)


@pytest.mark.parametrize('marcher', MARCHERS)
def test_kstep_counter_is_lower_with_order(engines, main_renders, marcher):
    """The k-steps the compacted 64-ray tiles executed, summed over the steps with rounds: fewer with the ordered list than with the
    atomic append (no margin: ordered tiles keep fewer k-steps than glued ones, the CPU count of profiles/live_order.md)."""
    tot = []
    for eng, r in zip(engines, main_renders[marcher]):
        counts, ks = _fine_counts(eng, r, KW[marcher])
        rounds = [s for s, c in enumerate(counts) if _round_step(c)]
        assert len(rounds) >= 2, counts           # (step 0 reads the same list in both modes)
        for s in rounds:
            tiles, done, dense = ks[s]
            assert tiles > 0 and dense == 768 * tiles and 0 < done <= dense, (s, ks[s])
        assert all(ks[s][0] == 0 for s in range(len(counts)) if not _round_step(counts[s])), ks      # (no 64-ray tiles elsewhere)
        tot.append((sum(ks[s][1] for s in rounds), sum(ks[s][2] for s in rounds)))
    print('k-steps over the round steps: ordered %d, appended %d, dense %d' % (tot[0][0], tot[1][0], tot[0][1]))
    assert tot[0][1] == tot[1][1]                 # the same tiles
    assert tot[0][0] < tot[1][0]


@pytest.mark.parametrize('marcher', MARCHERS)
def test_list_read_back(engines, main_renders, marcher):
    """distr_debug_live_list after the round steps, the regime's last step and one step beyond it."""
    import torch
    kw = KW[marcher]
    on, off = main_renders[marcher]
    counts, _ = _fine_counts(engines[0], on, kw)
    rounds = [s for s, c in enumerate(counts) if _round_step(c)]
    last = rounds[-1]
    assert rounds == list(range(last + 1)) and last + 2 < len(counts) and counts[last + 1] > 0, counts
    steps = sorted(set([0, last // 2, last, last + 1]))
    got = {}
    for mode, (eng, r) in enumerate(zip(engines, (on, off))):
        cfg = r['cfg']
        lat, Rs, Ts = (x.detach()[0].contiguous() for x in r['inputs'])
        ws = torch.empty(eng.ctx.workspace_bytes(cfg)[0], dtype=torch.uint8, device=eng.device)
        for run in range(2 if mode == 0 else 1):
            for s in steps:
                read, left, ordered = eng.ctx.debug_live_list(cfg, lat, Rs, Ts, s, ws)
                assert len(read) == counts[s] and len(left) == counts[s + 1], (s, len(read), len(left), counts)
                assert len(set(left.tolist())) == len(left) and len(set(read.tolist())) == len(read), 'duplicates in the list of step %d' % s
                assert set(left.tolist()) <= set(read.tolist())
                assert ordered == (mode == 0 and s <= last), (mode, s, ordered)
                if ordered:       # exactly the list the step read with the non-survivors struck out
                    stay = np.isin(read, left)
                    assert (read[stay] == left).all(), 'step %d: survivors out of order' % s
                got[(mode, run, s)] = left
    for s in steps:       # the same rays in both modes and in both runs
        assert (np.sort(got[(0, 0, s)]) == np.sort(got[(1, 0, s)])).all() and (np.sort(got[(0, 0, s)]) == np.sort(got[(0, 1, s)])).all(), s
    # the appended list of a step behind the first really is in another order (else the ordered assertion above would test nothing)
    read, left, _ = engines[1].ctx.debug_live_list(off['cfg'], *(x.detach()[0].contiguous() for x in off['inputs']), 1,
                                                   torch.empty(engines[1].ctx.workspace_bytes(off['cfg'])[0], dtype=torch.uint8, device=engines[1].device))
    print('atomic append, step 1: survivors in the order of the list read: %s' % bool((read[np.isin(read, left)] == left).all()))


def test_repeated_renders(engines, main_renders, fixture_decoder):
    """A configuration's later renders launch k_live_pack only up to the step at which the previous render left the round regime (+1; the
    hint k_finalize writes): the same bytes, and the round steps are still ordered."""
    m = 'pyramid_recursive'
    first_on, first_off = main_renders[m]
    for _ in range(2):
        again = _render(engines[0], fixture_decoder[2], H, W, [_camera()], KW[m])
        assert _diff(again, first_on) == []
    counts, ks = _fine_counts(engines[0], again, KW[m])
    _, ks_off = _fine_counts(engines[1], first_off, KW[m])
    rounds = [s for s, c in enumerate(counts) if _round_step(c)]
    assert sum(ks[s][1] for s in rounds) < sum(ks_off[s][1] for s in rounds)


@pytest.mark.parametrize('order', [0, 1])
def test_strip_enumeration_gives_the_same_bytes(main_renders, fixture_decoder, order):
    """DISTR_RAY_BLOCKS=0 (pixels in strips of 256, with DISTR_LIVE_ORDER=0 the schedule before the ordered list) against the blocks."""
    eng = _engine(fixture_decoder, DISTR_RAY_BLOCKS=0, DISTR_LIVE_ORDER=order)
    for m in MARCHERS:
        assert _diff(_render(eng, fixture_decoder[2], H, W, [_camera()], KW[m]), main_renders[m][0]) == [], m


def test_odd_image(engines, strips, fixture_decoder):
    """137 x 137: odd both ways (partial blocks on both edges, a partial last tile)."""
    a, b, c = (_render(e, fixture_decoder[2], 137, 137, [_camera()], KW['pyramid_recursive']) for e in engines + (strips,))
    assert _diff(a, b) == [] and _diff(a, c) == []
    assert engines[0].ctx.render_stats(a['node'].cfg, a['node'].ws)['num_in_sphere'] == 137 * 137
    assert _round_step(engines[0].ctx.live_counts(a['node'].cfg, a['node'].ws)[6])


def test_row_band(engines, strips, fixture_decoder):
    """Rows [4, 128) of the 136 x 144 image: the band's blocks start at its own first row; 124 rows = 7 block rows and 12 rows."""
    from distr import binding, fixture
    kw = KW['pyramid_recursive']
    with pytest.raises(binding.DistrError):
        engines[0].ctx.workspace_bytes(binding.make_cfg((H, W), fixture.make_intrinsic(H, W), band=(3, 124), **kw))
    a, b, c = (_render(e, fixture_decoder[2], H, W, [_camera()], kw, band=(4, 124)) for e in engines + (strips,))
    assert _diff(a, b) == [] and _diff(a, c) == []
    assert a['mask'].shape[-1] == 124 * W and engines[0].ctx.render_stats(a['node'].cfg, a['node'].ws)['num_in_sphere'] == 124 * W
    counts = engines[0].ctx.live_counts(a['node'].cfg, a['node'].ws)
    assert _round_step(counts[6]), counts       # (the band still has a round in its first full-resolution step)


def test_batch_of_two_views(engines, fixture_decoder):
    """Two cameras in one launch sequence: every view keeps its own list, slots and counts; each view equals its stand-alone render."""
    import helpers
    kw = KW['pyramid_recursive']
    cams = [helpers.bench_camera(0), helpers.bench_camera(3)]
    on, off = (_render(e, fixture_decoder[2], H, W, cams, kw) for e in engines)
    assert _diff(on, off) == []
    for v, cam in enumerate(cams):
        alone = _render(engines[0], fixture_decoder[2], H, W, [cam], kw)
        bad = [k for k in OUTS + GRADS if np.asarray(on[k][v]).tobytes() != np.asarray(alone[k][0]).tobytes()]
        assert bad == [], (v, bad)


@pytest.mark.parametrize('name,t32,t16', [('no_32_ray_role', 4096, 4096), ('remainder_on_64_ray_tiles', 64, 64)])
def test_tile_thresholds_leave_outputs_unchanged(engines, main_renders, fixture_decoder, name, t32, t16):
    """Ordered mode with other splits of a step's remainder: t32 = t16 removes the 32-ray role, t32 = t16 = 64 sends every remainder above
    128 rays to 64-ray tiles (more ordered steps, partial rounds)."""
    eng = _engine(fixture_decoder, DISTR_LIVE_ORDER=1, DISTR_HYBRID_THRESHOLD=t32, DISTR_TAIL16_THRESHOLD=t16)
    for m in MARCHERS:
        a = _render(eng, fixture_decoder[2], H, W, [_camera()], KW[m])
        assert _diff(a, main_renders[m][0]) == [], (name, m)
