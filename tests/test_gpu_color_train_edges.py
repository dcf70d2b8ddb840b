"""The generalised geometry of the layer-wise train path (distr_train_net_*) held byte for byte to its documented f32
chains, the way tests/test_gpu_train_edges.py holds the SDF decoder's: tests/color_train_exact_restatement.py restates the path on a few
probe rows -- segment ends, in-segment 63 / 64, workspace rows 127 / 128, two padded rows. Per case (the colour net of colour-code
length cs, L = 256 + cs, lin4's row stride ld4 = 512 + cs, on segments [1, 65, 0, 63, 64] = 320 rows, two K slabs):

  a  X_1..X_8 on the probe rows equal the chains; the three outputs are within 2e-6 of tanh of the exact z (the f32 tanh's bar of the
     SDF edge tests; z itself is pinned by d: dz = w (1 - s^2) comes from the saved tanh)
  b  a one-hot backward per probe point and channel reads dz[row][ch] from g_b8[ch] (zeros are added to it and nothing else; the other
     two channels stay exact zeros)
  c  one backward with the upstream gradient on the probe points only: all eighteen gradients and every g_latent row equal the
     restatement; g_W4's four column blocks [lin3 cols | shape | colour | xyz] and g_W0's three are all hit
  d  a run on a workspace and outputs pre-filled with 0xFF bytes gives the same bytes, all finite

cs = 1 (ld4 = 513: no float4 on W4, the xyz tail at an odd offset, k_train_glatent's second block with one live thread), 2, 3
(unaligned ld4), 4 (the smallest aligned ld4 after 512), 255, 256 (two full blocks of k_train_glatent, 516 entries per row in
k_train_bias), 257 (a third block). Then out_dim = 3 with a single point in all (M = 1 in every GEMM), and 64 segments of 65 (32 slabs).
"Equal bytes" counts +0 and -0 as equal. Mutation check and measured figures: profiles/color_train_edges.md."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F32 = np.float32
U = 2.0 ** -24
SEGS = [1, 65, 0, 63, 64]
COLOR_SIZES = (1, 2, 3, 4, 255, 256, 257)


def probe_rows(counts, around=(127, 128)):
    import color_train_exact_restatement as cx
    seg, idx, pt = cx.row_table(counts)
    seg_row = cx.train_segment_rows(counts)
    real = set()
    for s, n in enumerate(counts):
        if n:
            real |= {seg_row[s], seg_row[s] + n - 1} | {seg_row[s] + i for i in (63, 64) if i < n}
    real |= {r for r in around if r < len(pt) and pt[r] >= 0}
    padded = [r for r in range(len(pt)) if pt[r] < 0]
    behind = [r for r in padded if r > 0 and pt[r - 1] >= 0]
    return sorted(real), sorted(set(behind[:1] + padded[-1:]))


class Case(object):
    def __init__(self, cs, counts, real=None, pads=None):
        import color_train_exact_restatement as cx
        from distr import fixture
        self.cs, self.L, self.counts = cs, 256 + cs, list(counts)
        self.Ws, self.bs, cc0 = fixture.make_color_decoder_weights(color_size=cs)
        S, n = len(counts), sum(counts)
        rs = np.random.RandomState(4100 + cs + 17 * n)
        self.codes = np.concatenate([0.1 * rs.standard_normal((S, 256)), cc0 + 0.1 * rs.standard_normal((S, cs))], 1).astype(F32)
        self.pts = ((rs.rand(n, 3) - 0.5) * 1.6).astype(F32)
        self.w_dense = (1.0 + rs.standard_normal((n, 3))).astype(F32)
        self.seg, self.idx, self.pt = cx.row_table(counts)
        if real is None:
            real, pads = probe_rows(counts)
        self.real, self.pads = list(real), list(pads)
        assert all(self.pt[r] >= 0 for r in self.real) and all(self.pt[r] < 0 for r in self.pads) and len(self.real) <= 16
        self.rows = sorted(self.real + self.pads)
        self.w_probe = np.zeros((n, 3), F32)
        k = len(self.real)
        self.w_probe[self.pt[self.real]] = ((1.0 + rs.rand(k, 3)) * np.where(rs.rand(k, 3) < 0.5, -1, 1)).astype(F32)
        self._gpu = None

    def xyz_of(self, rows):
        rows = np.asarray(rows)
        return np.where(self.pt[rows][:, None] >= 0, self.pts[np.maximum(self.pt[rows], 0)], F32(0)).astype(F32)

    def gpu(self):
        import torch
        from distr import functions
        if self._gpu is None:
            g = dict(weights=[torch.from_numpy(a).cuda() for a in self.Ws + self.bs], codes=torch.from_numpy(self.codes).cuda(), pts=torch.from_numpy(self.pts).cuda())
            g['net'] = (self.L, 253, 3)
            assert functions.color_train_net(g['weights']) == g['net']
            g['rgb'], g['saved'] = functions.train_forward(g['weights'], g['codes'], g['pts'], self.counts, None, net=g['net'])
            self._gpu = g
        return self._gpu

    def backward(self, w):
        import torch
        from distr import functions
        grads, g_lat = functions.train_backward(self.gpu()['saved'], torch.from_numpy(np.asarray(w, F32)).cuda())
        return [g.cpu().numpy() for g in grads], g_lat.cpu().numpy()

    def saved_rows(self, rows):
        import torch
        saved = self.gpu()['saved']
        at = torch.as_tensor(list(rows)).cuda()
        return [None] + [saved.activations(l)[at].cpu().numpy() for l in range(1, 9)]


_cases = {}


def case_of(cs):
    if cs not in _cases:
        _cases[cs] = Case(cs, SEGS)
    return _cases[cs]


def check_forward_bytes(c):
    import color_train_exact_restatement as cx
    rows = np.asarray(c.rows)
    X, z = cx.forward_rows(c.Ws, c.bs, c.codes, c.seg[rows], c.idx[rows], c.xyz_of(rows))
    got = c.saved_rows(c.rows)
    assert got[4].shape[1] == 253 and z.shape == (len(rows), 3)
    for l in range(1, 9):
        if not cx.same_bytes(got[l], X[l]):
            bad = np.argwhere(got[l] != X[l])
            r, n = bad[0]
            raise AssertionError('cs %d: X_%d differs from the f32 chain at %d elements of %s; the first: workspace row %d, unit %d: GPU %r, chain %r'
                                 % (c.cs, l, len(bad), got[l].shape, c.rows[r], n, got[l][r, n], X[l][r, n]))
        assert (got[l] > 0).any() and (got[l] == 0).any(), (c.cs, l)
    at = [c.rows.index(r) for r in c.real]
    s = np.tanh(z[at].astype(np.float64))
    rgb = c.gpu()['rgb'].cpu().numpy()
    assert rgb.shape == (sum(c.counts), 3)
    d = np.abs(rgb[c.pt[c.real]] - s).max()
    print('cs %d: X_1..X_8 equal the f32 chains on rows %s; |rgb - tanh(exact z)| <= %.2e' % (c.cs, c.rows, d))
    assert d <= 2e-6, (c.cs, d)
    assert np.abs(s).max() < 0.999 and np.ptp(s) > 0.05, 'the probes are neither saturated nor all alike'


def probe_dz(c):
    """dz[probe][ch] from one one-hot backward each: g_b8[ch]; the other channels of g_b8 are exact zeros."""
    rgb = c.gpu()['rgb'].cpu().numpy()
    dz = np.zeros((len(c.real), 3), F32)
    for i, r in enumerate(c.real):
        p = c.pt[r]
        for ch in range(3):
            w1 = np.zeros_like(c.w_probe)
            w1[p, ch] = c.w_probe[p, ch]
            grads, _ = c.backward(w1)
            g_b8 = grads[17]
            assert g_b8.shape == (3,) and not np.delete(g_b8, ch).any(), (c.cs, r, ch, g_b8)
            dz[i, ch] = g_b8[ch]
            s, w = float(rgb[p, ch]), float(w1[p, ch])
            assert abs(float(dz[i, ch]) - w * (1 - s * s)) <= 3 * U * abs(w) * (1 + s * s), (c.cs, r, ch, dz[i, ch], w, s)
            assert dz[i, ch] != 0
    return dz


def check_backward_bytes(c):
    import color_train_exact_restatement as cx
    import color_train_restatement as cr
    dz = probe_dz(c)
    grads, g_lat = c.backward(c.w_probe)
    X = c.saved_rows(c.real)
    g_W, g_b, x_lat = cx.backward_rows(c.Ws, c.codes, c.counts, c.real, c.xyz_of(c.real), X, dz)
    for l in range(9):
        for name, got, ref in (('g_W%d' % l, grads[l], g_W[l]), ('g_b%d' % l, grads[9 + l], g_b[l])):
            if not cx.same_bytes(got, ref):
                bad = np.argwhere(got != ref)
                at = tuple(bad[0])
                raise AssertionError('cs %d: %s differs from the documented order at %d of %d elements; the first: %s: GPU %r, restatement %r'
                                     % (c.cs, name, len(bad), got.size, at, got[at], ref[at]))
    for name, i, cols in cr.gradient_blocks(c.cs):
        assert grads[i][..., cols].any(), (c.cs, name, 'not hit')
    for s, n in enumerate(c.counts):
        assert cx.same_bytes(g_lat[s], x_lat[s]), (c.cs, 'g_latent row', s, int((g_lat[s] != x_lat[s]).sum()))
        probed = bool((c.seg[c.real] == s).any())           # (a segment without a probe point has no upstream gradient)
        assert (g_lat[s, :256].any() and g_lat[s, 256:].any()) if probed else not g_lat[s].any(), (c.cs, s)
    print('cs %d: eighteen gradients and %d g_latent rows equal the restatement from probe rows %s' % (c.cs, len(c.counts), c.real))


@pytest.mark.parametrize('cs', COLOR_SIZES)
def test_a_forward_bytes(cs):
    check_forward_bytes(case_of(cs))


@pytest.mark.parametrize('cs', COLOR_SIZES)
def test_bc_backward_bytes(cs):
    check_backward_bytes(case_of(cs))


@pytest.mark.parametrize('cs', COLOR_SIZES)
def test_d_poison(cs):
    """An element a kernel fails to write, or a read beyond M, N or K, meets NaN (f32) / -1 (int32) instead of the last run's answer."""
    import torch
    from distr import functions
    c = case_of(cs)
    g = c.gpu()
    grads, g_lat = c.backward(c.w_dense)
    ws = torch.full_like(g['saved'].ws, 0xFF)
    rgb = torch.full_like(g['rgb'], float('nan'))
    out_g = [torch.full_like(w, float('nan')) for w in g['weights']]
    out_l = torch.full((len(c.counts), c.L), float('nan'), device='cuda')
    assert torch.isnan(ws.view(torch.float32)).all()
    rgb2, saved2 = functions.train_forward(g['weights'], g['codes'], g['pts'], c.counts, None, ws=ws, out=rgb, net=g['net'])
    assert rgb2 is rgb and saved2.ws is ws
    grads2, g_lat2 = functions.train_backward(saved2, torch.from_numpy(c.w_dense).cuda(), out=(out_g, out_l))
    assert grads2 is out_g and g_lat2 is out_l
    for tag, a, b in [('rgb', g['rgb'], rgb), ('g_latent', torch.from_numpy(g_lat).cuda(), out_l)] + [('gradient %d' % i, torch.from_numpy(grads[i]).cuda(), out_g[i]) for i in range(18)]:
        assert torch.isfinite(b).all(), (cs, tag, int((~torch.isfinite(b)).sum()))
        assert torch.equal(a, b), (cs, tag)
    _cases.pop(cs).__dict__.clear()          # (the last test of this case: release its workspace)


def test_a_single_point():
    """out_dim = 3 with one point in all: M = 1 in the forward and delta GEMMs, K = 64 rows (63 padded) in the weight gradients."""
    import color_train_exact_restatement as cx
    c = Case(3, [1], [0], [1, 63])
    rows = np.asarray(c.rows)
    X, z = cx.forward_rows(c.Ws, c.bs, c.codes, c.seg[rows], c.idx[rows], c.xyz_of(rows))
    got = c.saved_rows(c.rows)
    for l in range(1, 9):
        assert cx.same_bytes(got[l], X[l]), l
    assert np.abs(c.gpu()['rgb'].cpu().numpy()[0] - np.tanh(z[0].astype(np.float64))).max() <= 2e-6
    check_backward_bytes(c)


def test_large_64_segments_of_65():
    """8192 rows, 32 slabs, two blocks per segment; probes in segments 0, 7, 8 and 63: g_b and the xyz columns add 64 segments in order,
    the code columns of g_W0 / g_W4 chain over them."""
    from distr import functions
    counts = [65] * 64
    assert functions.train_slab_plan(functions.train_segment_rows(counts)[-1]) == (256, 32)
    real = [0, 63, 64] + [7 * 128, 7 * 128 + 64] + [8 * 128, 8 * 128 + 64] + [63 * 128, 63 * 128 + 64]
    c = Case(256, counts, real, [65, 8191])
    check_forward_bytes(c)
    check_backward_bytes(c)
