"""The layer-wise train path (distr_train_*, DESIGN.md sections 8f and 8g) held to its documented f32 chains at every tile edge.

tests/train_exact_restatement.py restates the path bit for bit on a few probe rows (tests/test_train_exact_host.py pins it on the CPU).
Per case:

  a  forward bytes: X_1..X_8 on the probe rows (real and padded) equal the restatement; sdf within 2e-6 of tanh of the exact z
  b  forward, every element, layer-local: from the GPU's saved X_l, |X_(l+1) - relu(pre)| <= (K + 4) 2^-24 S in float64, with
     pre = X_l W^T + b (lin0: [code, xyz]; lin4: [X_4, code, xyz]) and S the same sum of magnitudes -- the bound of a chain of K + 3
     fmas plus one term of margin; a dropped or doubled product is far above it
  c  poison: workspace and every output filled with 0xFF bytes beforehand (NaN as f32, -1 as int32): same bytes, all finite
  d  backward bytes: dz of every probe point from a one-hot backward (g_b8 is that dz: zeros are added to it and nothing else),
     each within 3 2^-24 |w| (1 + s^2) of w (1 - s^2) -- either contraction of the kernel's expression; then one backward with the
     upstream gradient on the probe points only: all eighteen gradients and every g_latent row equal the restatement byte for byte
  e  dense backward: against the float64 restatement with the GPU's gates, at 1e-4 of the largest entry of each BLOCK
     (train_restatement.gradient_blocks: the latent, xyz and activation columns of g_W0 / g_W4 come from different kernels)

"Equal bytes" counts +0 and -0 as equal. Decoders: the fixtures with non-zero biases (b_l += 0.05 N(0, 1), l < 8), so that the
accumulator's start is exercised. Code lengths: 509 - C = 1, 2, 3 (below one quad), 15, 16, 17 (one 16-deep stage -, =, +), 127 .. 131
(one 128-wide tile - 1 .. + 3: all four residues mod 4), 256 (two tiles), 508 -- both ends of the accepted range. Point list
[1, 65, 0, 63, 64]: 320 rows = two full 128-row tiles and a half-filled one, tiles 0 and 1 hold blocks of two segments each, one segment
is empty, two K slabs (256 + 64 rows; the one-segment lists of 257 and 513 points have the cut inside a segment). Then C = 380 with a
clamp, with a shared code, with dropout (also C = 494), on one segment of n points for n around 64, 128, 256 and 512 rows, and on two
large lists (sparse checks only). Measured figures: profiles/train_edges.md.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F32 = np.float32
U = 2.0 ** -24
CODE_LENGTHS = (508, 507, 506, 494, 493, 492, 382, 381, 380, 379, 378, 253, 1)
SEGS = [1, 65, 0, 63, 64]
ROW_EDGES = (1, 64, 65, 127, 128, 129, 255, 256, 257, 513)
SEED = 0x5EED0002

# name -> (C, counts, variant): variant 'plain', 'clamp' (0.1), 'shared' (one code), or a dropout (layers, p)
CASES = {'C%d' % Cn: (Cn, SEGS, 'plain') for Cn in CODE_LENGTHS}
CASES['C380-clamp'] = (380, SEGS, 'clamp')
CASES['C380-shared'] = (380, SEGS, 'shared')
MAIN = list(CASES)
EDGE = ['n%d' % n for n in ROW_EDGES]
CASES.update({'n%d' % n: (380, [n], 'plain') for n in ROW_EDGES})
DROP = []
for _Cn in (380, 494):
    for _tag, _layers, _p in (('all-p0.2', tuple(range(8)), 0.2), ('037-p0.5', (0, 3, 7), 0.5)):
        CASES['C%d-drop-%s' % (_Cn, _tag)] = (_Cn, SEGS, (_layers, _p))
        DROP.append('C%d-drop-%s' % (_Cn, _tag))
SEGMENT_BASE = 5


def decoder(Cn, dropout=None):
    """The fixture decoder of code length C with non-zero biases on lin0..lin7. With dropout the columns that read a dropped layer are
    multiplied by 1 - p (tests/test_gpu_train_dropout.py::_rescaled says why: the outputs stay away from the saturated tanh)."""
    from distr import fixture
    Ws, bs, latent = fixture.make_decoder_weights(latent_size=Cn)
    rs = np.random.RandomState(7000 + Cn)
    bs = [(b + 0.05 * rs.standard_normal(b.shape)).astype(F32) if l < 8 else b for l, b in enumerate(bs)]
    Ws = [np.array(W, dtype=F32) for W in Ws]
    if dropout is not None:
        layers, p = dropout
        for l in layers:
            if l + 1 == 4:
                Ws[4][:, :509 - Cn] *= F32(1 - p)
            else:
                Ws[l + 1] *= F32(1 - p)
    return Ws, bs, latent


def probe_rows(counts, around=(127, 128, 255, 256)):
    """(real probe rows, padded probe rows): per non-empty segment its first and last point and in-segment index 63 / 64; the points at
    the workspace rows `around`; padded: the row behind the first segment's last point that has one, and the list's last padded row."""
    import train_exact_restatement as ex
    seg, idx, pt = ex.row_table(counts)
    seg_row = ex.train_segment_rows(counts)
    real = set()
    for s, n in enumerate(counts):
        if n:
            real |= {seg_row[s], seg_row[s] + n - 1} | {seg_row[s] + i for i in (63, 64) if i < n}
    real |= {r for r in around if r < len(pt) and pt[r] >= 0}
    padded = [r for r in range(len(pt)) if pt[r] < 0]
    behind = [r for r in padded if r > 0 and pt[r - 1] >= 0]
    pads = sorted(set(behind[:1] + padded[-1:]))
    real = sorted(real)
    assert len(real) <= 16
    return real, pads


class Case(object):
    """One decoder, one point list, one variant: the inputs, and lazily the GPU forward, the restated forward and the backward runs."""

    def __init__(self, name, Cn, counts, variant, real=None, pads=None):
        import dropout_restatement as dr
        import train_exact_restatement as ex
        self.name, self.Cn, self.counts = name, Cn, list(counts)
        self.clamp = 0.1 if variant == 'clamp' else None
        drop = variant if isinstance(variant, tuple) else None
        self.Ws, self.bs, latent = decoder(Cn, drop)
        self.drop_gpu = self.drop_ex = None
        if drop is not None:
            layers, p = drop
            self.drop_gpu = (sum(1 << l for l in layers), dr.threshold(p), dr.scale(p), SEED, SEGMENT_BASE)
            self.drop_ex = (layers, dr.threshold(p), dr.scale(p), SEED, SEGMENT_BASE)
        S, n = len(counts), sum(counts)
        rs = np.random.RandomState(9000 + Cn + 17 * n)
        self.codes = (latent + 0.3 * np.abs(latent).max() * rs.standard_normal((1 if variant == 'shared' else S, Cn))).astype(F32)
        self.pts = ((rs.rand(n, 3) - 0.5) * 1.6).astype(F32)
        # the dense upstream gradient: N(1, 1). g_b8 is ONE number, sum_p w_p (1 - s_p^2), and a block's bar is relative to the block
        # itself. With these biases s is 0.93 .. 0.99, where the f32 tanh's half ulp (3e-8) is a relative 2 s 3e-8 / (1 - s^2) = 1e-6 ..
        # 4e-6 of every term; a sign-symmetric w makes the terms cancel (condition sum |t| / |sum t| of some 20 sqrt(n) / n ... 400 at
        # n = 194 for an unlucky draw), which puts that input error, not the summation order, at the 1e-4 bar. A mean of 1 keeps the
        # condition near 1.3 for every list; check_dense_backward asserts it from the float64 reference alone.
        self.w_dense = (1.0 + rs.standard_normal(n)).astype(F32)
        if variant == 'clamp':
            # with these biases the fixture's field is 0.93 .. 0.99 everywhere, all of it beyond the clamp: move b8 (which the biases
            # above leave alone) by the list's median z in float64, so that the points lie on both sides of +-0.1
            import train_restatement as tr
            y, _ = tr.forward(tr.to64(self.Ws), tr.to64(self.bs), tr.to64([self.codes])[0], tr.to64([self.pts])[0], self.counts)
            self.bs[8] = (self.bs[8] - np.median(np.arctanh(y.numpy()))).astype(F32)
        self.seg, self.idx, self.pt = ex.row_table(counts)
        if real is None:
            real, pads = probe_rows(counts, (63, 64, 127, 128, 255, 256, 511, 512))
        self.real, self.pads = list(real), list(pads)
        assert all(self.pt[r] >= 0 for r in self.real) and all(self.pt[r] < 0 for r in self.pads)
        self.rows = sorted(self.real + self.pads)
        self.w_probe = np.zeros(n, F32)
        self.w_probe[self.pt[self.real]] = (1.0 + rs.rand(len(self.real))).astype(F32) * np.where(rs.rand(len(self.real)) < 0.5, -1, 1)
        self._cache = {}

    def xyz_of(self, rows):
        rows = np.asarray(rows)
        return np.where(self.pt[rows][:, None] >= 0, self.pts[np.maximum(self.pt[rows], 0)], F32(0)).astype(F32)

    def gpu(self):
        """The device tensors and the plain forward: dict(weights, codes, pts, sdf, saved)"""
        import torch
        from distr import functions
        if 'gpu' not in self._cache:
            g = dict(weights=[torch.from_numpy(a).cuda() for a in self.Ws + self.bs], codes=torch.from_numpy(self.codes).cuda(), pts=torch.from_numpy(self.pts).cuda())
            g['sdf'], g['saved'] = functions.train_forward(g['weights'], g['codes'], g['pts'], self.counts, self.clamp, dropout=self.drop_gpu)
            self._cache['gpu'] = g
        return self._cache['gpu']

    def backward(self, w):
        """([18 gradients], g_latent) as numpy, from the cached forward"""
        import torch
        from distr import functions
        grads, g_lat = functions.train_backward(self.gpu()['saved'], torch.from_numpy(np.asarray(w, F32)).cuda())
        return [g.cpu().numpy() for g in grads], g_lat.cpu().numpy()

    def saved_rows(self, rows):
        """[None, X_1 .. X_8] of the GPU run on the given workspace rows, numpy"""
        import torch
        saved = self.gpu()['saved']
        at = torch.as_tensor(list(rows)).cuda()
        return [None] + [saved.activations(l)[at].cpu().numpy() for l in range(1, 9)]

    def exact_forward(self):
        import train_exact_restatement as ex
        if 'fwd' not in self._cache:
            rows = np.asarray(self.rows)
            self._cache['fwd'] = ex.forward_rows(self.Ws, self.bs, self.codes, self.seg[rows], self.idx[rows], self.xyz_of(rows), self.drop_ex)
        return self._cache['fwd']

    def release(self):
        self._cache.clear()


_cases = {}


def case_of(name):
    if name not in _cases:
        _cases[name] = Case(name, *CASES[name])
    return _cases[name]


def check_forward_bytes(c):
    import train_exact_restatement as ex
    X, z = c.exact_forward()
    got = c.saved_rows(c.rows)
    for l in range(1, 9):
        if not ex.same_bytes(got[l], X[l]):
            bad = np.argwhere(got[l] != X[l])
            r, n = bad[0]
            raise AssertionError('%s: X_%d differs from the f32 chain at %d elements of %s; the first: workspace row %d, unit %d: GPU %r, chain %r'
                                 % (c.name, l, len(bad), got[l].shape, c.rows[r], n, got[l][r, n], X[l][r, n]))
        if got[l].shape[1] >= 32 and c.drop_ex is None:
            assert (got[l] > 0).any() and (got[l] == 0).any(), (c.name, l)
    at = [c.rows.index(r) for r in c.real]
    s = np.tanh(z[at].astype(np.float64))
    if c.clamp is not None:
        s = np.clip(s, -c.clamp, c.clamp)
    sdf = c.gpu()['sdf'].cpu().numpy()[c.pt[c.real], 0]
    d = np.abs(sdf - s).max()
    print('%s: X_1..X_8 equal the f32 chains on rows %s; |sdf - tanh(exact z)| <= %.2e' % (c.name, c.rows, d))
    assert d <= 2e-6, (c.name, d)
    if c.drop_ex is not None:       # the mask did drop and keep positive units of each masked layer
        plain = ex.forward_rows(c.Ws, c.bs, c.codes, c.seg[c.rows], c.idx[c.rows], c.xyz_of(c.rows), None)[0]
        assert (X[1] == 0)[plain[1] > 0].any() and (X[1] > 0).any()


def probe_dz(c):
    """dz of every probe point, from one one-hot backward each: g_b8. Checked against float64 from the returned sdf."""
    sdf = c.gpu()['sdf'].cpu().numpy()[:, 0]
    dz = np.zeros(len(c.real), F32)
    for i, r in enumerate(c.real):
        p = c.pt[r]
        w1 = np.zeros_like(c.w_probe)
        w1[p] = c.w_probe[p]
        grads, _ = c.backward(w1)
        dz[i] = grads[17][0]
        s, w = float(sdf[p]), float(c.w_probe[p])
        if c.clamp is not None and abs(s) >= c.clamp:
            # the returned value is clamped: the unclamped one is beyond the clamp (or on it), where dz is an exact zero -- unless it
            # sits on the clamp exactly, which the clamp case's points do not (asserted by its test)
            assert dz[i] == 0, (c.name, r, dz[i])
        else:
            assert abs(float(dz[i]) - w * (1 - s * s)) <= 3 * U * abs(w) * (1 + s * s), (c.name, r, dz[i], w, s)
            assert dz[i] != 0, (c.name, r)
    return dz


def check_backward_bytes(c):
    import train_exact_restatement as ex
    dz = probe_dz(c)
    grads, g_lat = c.backward(c.w_probe)
    X = c.saved_rows(c.real)
    g_W, g_b, x_lat, _ = ex.backward_rows(c.Ws, c.codes, c.counts, c.real, c.xyz_of(c.real), X, dz, c.drop_ex)
    for l in range(9):
        for name, got, ref in (('g_W%d' % l, grads[l], g_W[l]), ('g_b%d' % l, grads[9 + l], g_b[l])):
            if not ex.same_bytes(got, ref):
                bad = np.argwhere(got != ref)
                at = tuple(bad[0])
                raise AssertionError('%s: %s differs from the documented order at %d of %d elements; the first: %s: GPU %r, restatement %r'
                                     % (c.name, name, len(bad), got.size, at, got[at], ref[at]))
            assert got.any() or not dz.any(), (c.name, name)
    for s, n in enumerate(c.counts):
        assert ex.same_bytes(g_lat[s], x_lat[s]), (c.name, 'g_latent row', s, int((g_lat[s] != x_lat[s]).sum()))
        assert n > 0 or not g_lat[s].any(), (c.name, 'the empty segment has a code gradient')
    print('%s: eighteen gradients and %d g_latent rows equal the restatement from probe rows %s' % (c.name, len(c.counts), c.real))


def check_dense_backward(c):
    import torch
    import train_restatement as tr
    grads, g_lat = c.backward(c.w_dense)
    saved = c.gpu()['saved']
    idx = torch.cat([torch.arange(*saved.rows(s)) for s in range(len(c.counts))]).cuda()
    gates = [(saved.activations(l + 1)[idx] > 0).cpu() for l in range(8)]
    codes = np.repeat(c.codes, len(c.counts), 0) if c.codes.shape[0] == 1 else c.codes
    y, _, ref_W, ref_b, ref_rows = tr.gradients(c.Ws, c.bs, codes, c.pts, c.counts, c.w_dense, c.clamp, gates=gates)
    t = c.w_dense.astype(np.float64) * (1 - y.numpy()[:, 0] ** 2) * (1.0 if c.clamp is None else np.abs(y.numpy()[:, 0]) < c.clamp)
    assert np.abs(t).sum() <= 4 * abs(t.sum()), (c.name, 'the one-number block g_b8 is a cancelling sum: judge it with another upstream gradient')
    res =tr.blockwise_residuals(grads, [t.numpy() for t in ref_W + ref_b], c.Cn)
    for s, n in enumerate(c.counts):
        ref = ref_rows[s].numpy()
        top = np.abs(ref).max()
        if n == 0 or top == 0:
            assert not g_lat[s].any(), (c.name, s)
        else:
            res.append(('g_latent row %d' % s, np.abs(g_lat[s] - ref).max() / top, top))
    worst = max(res, key=lambda t: t[1])
    print('%s: dense backward, worst block %s: %.3e of its largest entry (%.3e)' % (c.name, worst[0], worst[1], worst[2]))
    for name, rel, top in res:
        assert rel <= 1e-4, (c.name, name, rel, top)
    return worst


@pytest.mark.parametrize('name', MAIN + EDGE + DROP)
def test_a_forward_bytes(name):
    check_forward_bytes(case_of(name))


@pytest.mark.parametrize('name', MAIN)
def test_b_forward_every_element(name):
    import torch
    c = case_of(name)
    g = c.gpu()
    saved = g['saved']
    n3 = 509 - c.Cn
    W64 = [torch.from_numpy(W).double().cuda() for W in c.Ws]
    b64 = [torch.from_numpy(b).double().cuda() for b in c.bs]
    rows = len(c.seg)
    codes = np.repeat(c.codes, len(c.counts), 0) if c.codes.shape[0] == 1 else c.codes
    inp = torch.from_numpy(np.concatenate([codes[c.seg], c.xyz_of(np.arange(rows))], 1)).double().cuda()
    ambiguous, total = 0, 0
    x = inp
    for l in range(9):
        if l == 4:
            x = torch.cat([x, inp], 1)
        pre = x @ W64[l].t() + b64[l]
        bound = (x.shape[1] + 4) * U * (x.abs() @ W64[l].abs().t() + b64[l].abs())
        if l == 8:
            s = torch.tanh(pre[:, 0])
            if c.clamp is not None:
                s = s.clamp(-c.clamp, c.clamp)
            real = torch.from_numpy(np.nonzero(c.pt >= 0)[0]).cuda()
            d = (g['sdf'][:, 0].double() - s[real]).abs().max().item()
            assert d <= 2e-6, (name, d)
            break
        got = saved.activations(l + 1).double()
        if l == 3:
            assert got.shape[1] == n3
        err = (got - pre.clamp(min=0)).abs()
        over = err > bound
        if over.any():
            r, n = [int(v) for v in over.nonzero()[0]]
            raise AssertionError('%s: lin%d, row %d unit %d: GPU %r, float64 %r, bound %.3e (%d elements over the bound)'
                                 % (name, l, r, n, got[r, n].item(), pre[r, n].item(), bound[r, n].item(), int(over.sum())))
        ambiguous += int((pre.abs() <= bound).sum())
        total += pre.numel()
        if got.shape[1] >= 32:
            assert (got > 0).any() and (got == 0).any(), (name, l)
        x = got
    print('%s: %d of %d units have a pre-activation inside the bound (either side of the relu is right); |sdf - tanh| <= %.2e' % (name, ambiguous, total, d))


@pytest.mark.parametrize('name', MAIN)
def test_c_poison(name):
    """An element that a kernel fails to write, or a read beyond M, N or K, meets NaN (f32) / -1 (int32) instead of the last run's
    right answer in a recycled block."""
    import torch
    from distr import functions
    c = case_of(name)
    g = c.gpu()
    grads, g_lat = c.backward(c.w_dense)
    ws = torch.full_like(g['saved'].ws, 0xFF)
    sdf = torch.full_like(g['sdf'], float('nan'))
    out_g = [torch.full_like(w, float('nan')) for w in g['weights']]
    out_l = torch.full((len(c.counts), c.Cn), float('nan'), device='cuda')
    assert torch.isnan(ws.view(torch.float32)).all() and (ws.view(torch.int32) == -1).all()
    sdf2, saved2 = functions.train_forward(g['weights'], g['codes'], g['pts'], c.counts, c.clamp, ws=ws, out=sdf)
    assert sdf2 is sdf and saved2.ws is ws
    grads2, g_lat2 = functions.train_backward(saved2, torch.from_numpy(c.w_dense).cuda(), out=(out_g, out_l))
    assert grads2 is out_g and g_lat2 is out_l
    for tag, a, b in [('sdf', g['sdf'], sdf), ('g_latent', torch.from_numpy(g_lat).cuda(), out_l)] + [('gradient %d' % i, torch.from_numpy(grads[i]).cuda(), out_g[i]) for i in range(18)]:
        assert torch.isfinite(b).all(), (name, tag, int((~torch.isfinite(b)).sum()))
        assert torch.equal(a, b), (name, tag)


@pytest.mark.parametrize('name', MAIN + EDGE + DROP)
def test_d_backward_bytes(name):
    c = case_of(name)
    if name == 'C380-clamp':
        s = c.gpu()['sdf'].cpu().numpy()[c.pt[c.real], 0]
        assert (np.abs(s) == F32(0.1)).any() and (np.abs(s) < F32(0.1)).any(), s       # a probe outside the clamp, and one inside
    check_backward_bytes(c)


@pytest.mark.parametrize('name', MAIN + EDGE)
def test_e_dense_backward_blockwise(name):
    check_dense_backward(case_of(name))


def _large(name, Cn, counts, real, plan):
    from distr import functions
    assert functions.train_slab_plan(functions.train_segment_rows(counts)[-1]) == plan
    c = Case(name, Cn, counts, 'plain', real, [])
    try:
        check_forward_bytes(c)
        check_backward_bytes(c)
    finally:
        c.release()


def test_large_64_segments_of_65():
    """8192 rows, 32 slabs; two blocks per segment. Probes in segments 0, 7, 8 and 63: g_b and the xyz columns add 64 segments in
    order, the latent columns chain over them."""
    real = [0, 63, 64] + [7 * 128, 7 * 128 + 64] + [8 * 128, 8 * 128 + 64] + [63 * 128, 63 * 128 + 64]
    _large('64x65', 380, [65] * 64, real, (256, 32))


def test_large_one_segment_of_16385():
    """16 448 rows: the first row count with a slab longer than 256 (320 x 52), 257 blocks in one segment (lane j takes 32 or 33)."""
    _large('1x16385', 380, [16385], [0, 319, 320, 16319, 16320, 16384], (320, 52))
