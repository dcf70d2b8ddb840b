"""The split arithmetics (arith='bf16x6', arith='f16x3') against float64: forward, the range of the f16 form, the backward's dX
chain on single-sample probes, and the backward's additivity. References: tests/train_restatement.py (float64 decoder and its
gradients), tests/split_restatement.py (plane-exact CPU models, the rescaled decoders), the CPU oracle (sample points and
coefficients of a render's backward). The measured figures are recorded in DESIGN.md section 4.

Bars. (a) a split mode's max |sdf - sdf64| and its 99th percentile may be at most 2 x the f32 kernel's on the same points (2 x a
floor is the project's convention; tests/test_split_arith_host.py shows on the CPU model that a correct tile sits at 0.8 .. 1.1 of
the f32 error and a tile that lost any one product at 6.8 x or more). (c) a probe's residual may be at most 3 x the largest
residual of the f32 kernel over the probes. (d) an additivity residual may be at most 4 x the f32 kernel's.
"""
import numpy as np
import pytest

import helpers
import split_restatement as sr
import train_restatement as tr

pytestmark = pytest.mark.gpu

MODES = ('bf16x6', 'f16x3')
BAR = 2.0
NPTS = 8193                     # 129 tiles of 64, the last with one point
CODES = (None, 1235, 1236)      # the fixture's code, fixture.make_latent(seed)


def _f64(Ws, bs, latent, pts, clamp=None):
    import torch
    with torch.no_grad():
        return tr.forward(tr.to64(Ws), tr.to64(bs), tr.to64([latent])[0], tr.to64([pts])[0], [len(pts)], clamp)[0].reshape(-1).numpy()


def _eval(eng, latent, pts, arith, clamp=None):
    import torch
    from distr import functions
    out = functions.mlp_eval(eng, torch.from_numpy(latent).cuda(), torch.from_numpy(pts).cuda(), clamp_dist=clamp, arith=arith)
    return out.reshape(-1).cpu().numpy()


def _errors(sdf, ref, keep=None):
    e = np.abs(sdf.astype(np.float64) - ref)
    if keep is not None:
        e = e[keep]
    return float(e.max()), float(np.percentile(e, 99))


@pytest.fixture(scope='module')
def points():
    return (np.random.RandomState(11).rand(NPTS, 3) * 1.6 - 0.8).astype(np.float32)


@pytest.fixture(scope='module')
def decoders(fixture_decoder):
    from distr import fixture
    return {'f1': fixture_decoder, 'f2': fixture.load_fixture_f2()}


@pytest.fixture(scope='module')
def engines(decoders, engine):
    from distr import functions
    return {'f1': engine, 'f2': functions.engine_from_weights(decoders['f2'][0], decoders['f2'][1], 0)}


# ------------------------------------------------------------------------------------------------ (a) forward against float64
@pytest.mark.parametrize('code', CODES)
@pytest.mark.parametrize('fix', ['f1', 'f2'])
def test_forward_against_float64(decoders, engines, points, fix, code):
    """Each split mode's error against the float64 decoder is at most 2 x the f32 kernel's (max and 99th percentile), with and without
    the clamp; a shorter list (1, 63, 64, 65 points: a lone ray, one short of a tile, a tile, one over) returns the bytes of the long
    list's first points -- a ray's value does not depend on the rays that share its tile. Prints the distance to the CPU model."""
    from distr import fixture
    Ws, bs, latent = decoders[fix]
    if code is not None:
        latent = fixture.make_latent(code)
    eng = engines[fix]
    for clamp in (None, 0.05):
        ref = _f64(Ws, bs, latent, points, clamp)
        a = _eval(eng, latent, points, 'f32', clamp)
        e32 = _errors(a, ref)
        for arith in MODES:
            b = _eval(eng, latent, points, arith, clamp)
            e = _errors(b, ref)
            print('%s code %s clamp %s %s: max %.3e p99 %.3e | f32 kernel max %.3e p99 %.3e | ratios %.2f %.2f'
                  % (fix, code, clamp, arith, e[0], e[1], e32[0], e32[1], e[0] / e32[0], e[1] / e32[1]))
            assert np.isfinite(b).all()
            assert e[0] <= BAR * e32[0] and e[1] <= BAR * e32[1], (fix, code, clamp, arith, e, e32)
            if clamp is not None:
                assert np.abs(b).max() <= np.float32(clamp)
            for n in (1, 63, 64, 65):
                assert np.array_equal(_eval(eng, latent, points[:n], arith, clamp), b[:n]), (arith, n)
            if clamp is None and code is None:
                m = sr.forward(Ws, bs, latent, points, arith)[0].numpy()
                line = '%s %s: max |sdf_gpu - sdf_model| %.3e' % (fix, arith, np.abs(b - m).max())
                if arith == 'f16x3':
                    z = sr.forward(Ws, bs, latent, points, arith, ftz=True)[0].numpy()
                    line += ', against a model that flushes f16 denormals %.3e (that model against float64: %.3e)' % (np.abs(b - z).max(), _errors(z, ref)[0])
                print(line)


@pytest.mark.parametrize('arith', MODES)
def test_eval_value_is_independent_of_column_and_company(decoders, engines, points, arith):
    """The claim of the split tile's header for the point-list entry: a point's sdf depends neither on the column of the 64-ray tile it
    lands in nor on the points that share its tile. 97 points (one full tile and a tail of 33): the same bytes from one call, from the
    same points in reversed order (every point in another tile and column), and from the chunks [0:1], [1:34], [34:97]."""
    _, _, latent = decoders['f1']
    eng, pts = engines['f1'], points[:97]
    whole = _eval(eng, latent, pts, arith)
    assert np.isfinite(whole).all()
    reverse = _eval(eng, latent, np.ascontiguousarray(pts[::-1]), arith)[::-1]
    chunks = np.concatenate([_eval(eng, latent, pts[a:b], arith) for a, b in ((0, 1), (1, 34), (34, 97))])
    assert whole.tobytes() == reverse.tobytes(), np.flatnonzero(whole != reverse)
    assert whole.tobytes() == chunks.tobytes(), np.flatnonzero(whole != chunks)


# ------------------------------------------------------------------------------------------------ (b) the range of f16x3
def _single_weight(Ws, bs, value):
    W1 = [w.copy() for w in Ws]
    W1[2][5, 7] = value
    return W1, [b.copy() for b in bs]


def _members(Ws, bs):
    return [(n, W, b, None) for n, W, b in sr.family(Ws, bs)] + [('lin2 weight 1023', ) + _single_weight(Ws, bs, 1023.0) + (True,),
                                                                   ('lin2 weight 1024', ) + _single_weight(Ws, bs, 1024.0) + (False,)]


MEMBER_NAMES = [m[0] for m in _members([np.zeros((8, 8), np.float32)] * 9, [np.zeros(8, np.float32)] * 9)]


@pytest.fixture(scope='module')
def f1_ref(decoders, points):
    Ws, bs, latent = decoders['f1']
    return _f64(Ws, bs, latent, points)


def _small_render(eng, latent, arith):
    from distr import fixture
    H = W = 16
    return helpers.hip_render(eng, H, W, fixture.make_intrinsic(H, W), *fixture.make_camera(20.0, 10.0, 1.6, 0.0), latent, arith=arith,
                              march_step=6, buffer_size=2, marcher='recursive', use_depth2normal=True)


@pytest.mark.parametrize('member', MEMBER_NAMES)
def test_f16x3_range(decoders, points, f1_ref, member):
    """Function-preserving rescales of F1 by powers of two (the same float64 function, smaller activations in one layer or in six),
    and a single weight at the edge of the f16 range. f16x3 either meets bar (a), or refuses the decoder (from mlp_eval and from a
    render), or reports (NaN): it never returns finite values outside the bar. bf16x6 has f32's exponent range: bar (a), always.
    The library refuses exactly the decoders split_restatement.h3_refused_layer does, and names that layer."""
    from distr import binding, functions
    Ws0, bs0, latent = decoders['f1']
    name, Ws, bs, accept = [m for m in _members(Ws0, bs0) if m[0] == member][0]
    ref = f1_ref if accept is None else _f64(Ws, bs, latent, points)          # (a rescale keeps the float64 function exactly)
    eng = functions.engine_from_weights(Ws, bs, 0)
    e32 = _errors(_eval(eng, latent, points, 'f32'), ref)
    b6 = _eval(eng, latent, points, 'bf16x6')
    e6 = _errors(b6, ref)
    assert np.isfinite(b6).all() and e6[0] <= BAR * e32[0] and e6[1] <= BAR * e32[1], (name, e6, e32)
    try:
        h3 = _eval(eng, latent, points, 'f16x3')
    except binding.DistrError as err:
        print('%s: f32 max %.3e p99 %.3e | bf16x6 %.3e %.3e | f16x3 REFUSED: %s' % (name, e32[0], e32[1], e6[0], e6[1], err))
        assert accept is not True, name
        assert 'f16x3' in str(err) and sr.h3_refused_layer(Ws) is not None and ("lin%d's" % sr.h3_refused_layer(Ws)) in str(err), err
        with pytest.raises(binding.DistrError, match='f16x3'):
            _small_render(eng, latent, 'f16x3')
        _small_render(eng, latent, 'bf16x6')
        return
    assert accept is not False and sr.h3_refused_layer(Ws) is None, name
    fin = np.isfinite(h3)
    assert np.isnan(h3[~fin]).all()
    print('%s: largest weight %.1f | f32 max %.3e p99 %.3e | bf16x6 %.3e %.3e (ratio %.2f) | f16x3 reported %d points' %
          (name, max(float(np.abs(w).max()) for w in Ws[1:8]), e32[0], e32[1], e6[0], e6[1], e6[0] / e32[0], int((~fin).sum())), end='')
    if accept is True:
        assert fin.all()
    if fin.any():
        e3, e32f = _errors(h3, ref, fin), _errors(_eval(eng, latent, points, 'f32'), ref, fin)
        print(', the others max %.3e p99 %.3e (ratios %.2f %.2f)' % (e3[0], e3[1], e3[0] / e32f[0], e3[1] / e32f[1]))
        assert e3[0] <= BAR * e32f[0] and e3[1] <= BAR * e32f[1], (name, e3, e32f)


# ------------------------------------------------------------------------------------------------ (c) backward, single-sample probes
PROBE = dict(H=32, W=32, camera=(20, 10, 1.6, 0), kw=dict(marcher='recursive', march_step=30, buffer_size=2, want_normal=False), seed=2,
             n=256, views=64, gate_margin=1e-5, min_survivors=64)


@pytest.fixture(scope='module')
def probes(decoders, cpu_oracle, orc):
    """256 pixels of one 32 x 32 render (half hits, half misses, fixed seed), pixel i with the min-sdf gradient +-2^e, e running over
    -40..40: by the oracle's rule (k == 0 && grad_mask) each makes exactly one gradient sample. Per probe: the sample's point and
    coefficient from the oracle, the float64 gradient to the code on the oracle's ReLU pattern (the f32 kernel's: it is bit-identical)
    and on float64's own, and whether any of the 4 096 float64 pre-activations lies within 1e-5 of zero."""
    import torch
    from distr import fixture
    Ws, bs, latent = decoders['f1']
    H, W = PROBE['H'], PROBE['W']
    K = fixture.make_intrinsic(H, W)
    R, T = fixture.make_camera(*PROBE['camera'])
    out = cpu_oracle.render(orc.make_cfg(H, W, K, **PROBE['kw']), latent, R, T)
    rs = np.random.RandomState(PROBE['seed'])
    mask = out['mask'].astype(bool)
    hits, misses = np.flatnonzero(mask), np.flatnonzero(~mask)
    pix = np.concatenate([rs.choice(hits, PROBE['n'] // 2, replace=False), rs.choice(misses, PROBE['n'] // 2, replace=False)])
    pix = pix[rs.permutation(PROBE['n'])]
    weight = (rs.choice([-1.0, 1.0], PROBE['n']) * 2.0 ** (np.arange(PROBE['n']) % 81 - 40)).astype(np.float32)
    pts, coef = np.zeros((PROBE['n'], 3), np.float32), np.zeros(PROBE['n'], np.float32)
    for i in range(PROBE['n']):
        g = np.zeros(H * W, np.float32)
        g[pix[i]] = weight[i]
        p, x, c = out['state'].samples(g_min_sdf=g)
        assert p.tolist() == [pix[i]] and c[0] == weight[i], (i, p, c)
        pts[i], coef[i] = x[0], c[0]
    codes = np.repeat(latent, PROBE['n'], 0)
    gates = [torch.from_numpy(cpu_oracle.layer_activations(latent, pts, l)[:, :Ws[l].shape[0]] > 0) for l in range(8)]
    ref_f32 = tr.gradients(Ws, bs, codes, pts, [1] * PROBE['n'], coef, gates=gates)[4].numpy()
    _, pre, _, _, ref_own = tr.gradients(Ws, bs, codes, pts, [1] * PROBE['n'], coef)
    margin = torch.stack([z.abs().min(1).values for z in pre]).min(0).values.numpy()
    survive = margin >= PROBE['gate_margin']
    assert sum(z.shape[1] for z in pre) == 7 * 512 + 253              # the 4 096 units of the tile less lin3's padded rows
    return dict(K=K, R=R, T=T, latent=latent, pix=pix, weight=weight, pts=pts, coef=coef, ref_f32=ref_f32, ref_own=ref_own.numpy(),
                survive=survive, mask=mask)


def _probe_render(eng, arith, p, G, kw=None, H=None, K=None):
    """One render_batch_call of len(G) views of the probe camera with a code row per view; upstream gradient: G[v] on min_sdf (or on
    zdepth: kw / H / K given). Returns (g_latent (B, 256), g_R (B, 3, 3), g_T (B, 3), per-view num_grad_samples) as float64 / ints."""
    import torch
    from distr import binding, functions
    H = H or PROBE['H']
    cfg = binding.make_cfg((H, H), p['K'] if K is None else K, arith=arith, **(kw or PROBE['kw']))
    B = len(G)
    dev = eng.device
    lat = torch.from_numpy(np.repeat(p['latent'], B, 0)).to(dev).requires_grad_(True)
    R = torch.from_numpy(np.repeat(p['R'][None].astype(np.float32), B, 0)).to(dev).requires_grad_(True)
    T = torch.from_numpy(np.repeat(p['T'][None].astype(np.float32), B, 0)).to(dev).requires_grad_(True)
    zdepth, mask, min_sdf, _, _ = functions.render_batch_call(eng, cfg, lat, R, T)
    node = min_sdf.grad_fn
    Gt = torch.from_numpy(np.ascontiguousarray(G, np.float32)).to(dev)
    ((min_sdf if kw is None else zdepth) * Gt).sum().backward()
    torch.cuda.synchronize()
    counts = [eng.ctx.render_stats(node.cfg, node.ws[v * node.view_bytes:])['num_grad_samples'] for v in range(B)]
    return lat.grad.double().cpu().numpy(), R.grad.double().cpu().numpy(), T.grad.double().cpu().numpy(), counts


_probe_runs = {}


def _run_probes(eng, arith, p, key):
    """The 256 single-pixel probes in four calls of 64 views -> g_latent (256, 256), g_R (256, 3, 3), g_T (256, 3) per probe."""
    if (key, arith) not in _probe_runs:
        P = PROBE['H'] * PROBE['W']
        parts = []
        for c in range(PROBE['n'] // PROBE['views']):
            idx = np.arange(c * PROBE['views'], (c + 1) * PROBE['views'])
            G = np.zeros((PROBE['views'], P), np.float32)
            G[np.arange(PROBE['views']), p['pix'][idx]] = p['weight'][idx]
            parts.append(_probe_render(eng, arith, p, G))
            assert parts[-1][3] == [1] * PROBE['views'], parts[-1][3]
        _probe_runs[(key, arith)] = tuple(np.concatenate([q[i] for q in parts]) for i in range(3))
    return _probe_runs[(key, arith)]


def _probe_residuals(g_lat, ref):
    return np.abs(g_lat - ref).max(1) / np.abs(ref).max(1)


@pytest.fixture(scope='module')
def probe_floor(engine, probes):
    """arith='f32': every probe against float64 on the oracle's gates, no carve-out; the largest residual is the floor."""
    g_lat, _, _ = _run_probes(engine, 'f32', probes, 'f1')
    res = _probe_residuals(g_lat, probes['ref_f32'])
    print('f32 probes: largest residual %.3e of the probe\'s largest entry (median %.3e); hits %d, misses %d'
          % (res.max(), np.median(res), int(probes['mask'][probes['pix']].sum()), int((~probes['mask'][probes['pix']]).sum())))
    assert np.isfinite(g_lat).all()
    return float(res.max())


def test_probes_f32_match_float64(probe_floor, probes):
    assert int(probes['mask'][probes['pix']].sum()) == PROBE['n'] // 2
    # float64 on the f32 kernel's own ReLU pattern: what remains is f32 rounding of a 9-layer chain, far below 1e-4
    assert probe_floor <= 1e-4, probe_floor


def _check_split_probes(eng, arith, probes, floor, key):
    g_lat, _, _ = _run_probes(eng, arith, probes, key)
    s = probes['survive']
    res = _probe_residuals(g_lat, probes['ref_own'])
    print('%s %s probes: %d of %d survive the 1e-5 gate margin; largest residual of the survivors %.3e (f32 floor %.3e, ratio %.2f), of the others %.3e'
          % (key, arith, int(s.sum()), len(s), res[s].max(), floor, res[s].max() / floor, res[~s].max() if (~s).any() else 0.0))
    assert int(s.sum()) >= PROBE['min_survivors']
    assert np.isfinite(g_lat).all()
    assert res[s].max() <= 3.0 * floor, (arith, float(res[s].max()), floor, np.flatnonzero(s & (res > 3.0 * floor)))


@pytest.mark.parametrize('arith', MODES)
def test_probes_split_match_float64(engine, probes, probe_floor, arith):
    """split_backward in both formats on one sample per view, upstream gradients from 2^-40 to 2^40: every probe whose ReLU pattern
    is unambiguous (no float64 pre-activation within 1e-5 of zero: the forward's sample point differs from the oracle's by the march's
    1e-6-level drift) is within 3 x the f32 floor of float64."""
    _check_split_probes(engine, arith, probes, probe_floor, 'f1')


CHAIN_K = 6       # the largest k of the chain family that test_f16x3_range shows accepted and inside bar (a)


@pytest.mark.parametrize('arith', MODES)
def test_probes_split_on_small_activations(decoders, probes, probe_floor, arith):
    """The same probes on the chain-family decoder of k = 6 (the same function, exactly; activations of lin1..lin6 64 times smaller,
    so the normalised deltas of the backward are 64 times larger: closest to the f16 limit): finite, same bar."""
    from distr import functions
    Ws, bs = sr.rescale_chain(decoders['f1'][0], decoders['f1'][1], CHAIN_K)
    _check_split_probes(functions.engine_from_weights(Ws, bs, 0), arith, probes, probe_floor, 'chain')


# ------------------------------------------------------------------------------------------------ (d) backward, additivity
def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


EPS32 = 2.0 ** -24        # an f32 result cannot be closer to a float64 sum than its own rounding: the floor of the additivity bars


@pytest.fixture(scope='module')
def additivity_floor(engine, probes):
    return _additivity(engine, 'f32', probes)


def _additivity(eng, arith, p):
    """(i) one view with 48 of the probe pixels at once against the float64 sum of the 48 single probes; (ii) one dense 128 x 128
    pyramid view against the float64 sum of 8 views that keep an eighth of its pixels each. Relative residuals of (g_latent, g_R, g_T)."""
    from distr import fixture
    singles = _run_probes(eng, arith, p, 'f1')
    idx = np.arange(48)
    G = np.zeros((1, PROBE['H'] * PROBE['W']), np.float32)
    G[0, p['pix'][idx]] = p['weight'][idx]
    many = _probe_render(eng, arith, p, G)
    assert many[3] == [48]
    res_i = tuple(_rel(many[i][0], singles[i][idx].sum(0)) for i in range(3))
    H = 128
    kw = dict(marcher='pyramid_recursive', march_step=50, buffer_size=3, want_normal=False)
    gz = np.random.RandomState(21).randn(H * H).astype(np.float32)
    G = np.zeros((9, H * H), np.float32)
    G[0] = gz
    for j in range(8):
        G[1 + j, j::8] = gz[j::8]
    out = _probe_render(eng, arith, p, G, kw=kw, H=H, K=fixture.make_intrinsic(H, H))
    counts = out[3]
    assert counts[0] > 16384 and max(counts[1:]) <= 8192 and sum(counts[1:]) == counts[0], counts
    res_ii = tuple(_rel(out[i][0], out[i][1:].sum(0)) for i in range(3))
    print('%s additivity: (i) 48 probes at once: g_latent %.3e g_R %.3e g_T %.3e | (ii) %d samples against parts of %s: g_latent %.3e g_R %.3e g_T %.3e'
          % ((arith,) + res_i + (counts[0], counts[1:]) + res_ii))
    assert all(np.isfinite(o).all() for o in out[:3] + many[:3])
    return res_i, res_ii


def test_additivity_f32(additivity_floor):
    """The tile sizes of the exact path are pinned bit for bit per ray, so what differs is the order of the sums: f32 rounding."""
    for res in additivity_floor:
        assert max(res) <= 1e-5, additivity_floor


@pytest.mark.parametrize('arith', MODES)
def test_additivity_split(engine, probes, additivity_floor, arith):
    """The backward is linear in the upstream gradient and the forward is bit-reproducible: a view with many gradient pixels equals
    the float64 sum of the views that carry them one by one (tiles with several rays and unequal d8, the row sums of sd0 / sd4), and a
    view that sends whole rounds to the 64-sample kernel equals the sum of parts that run on 32-sample tiles only. Bar: 4 x the f32
    kernel's residual (at least 4 x 2^-24: the rounding of the f32 result itself)."""
    got = _additivity(engine, arith, probes)
    for res, floor in zip(got, additivity_floor):
        for r, f in zip(res, floor):
            assert r <= 4.0 * max(f, EPS32), (arith, got, additivity_floor)
