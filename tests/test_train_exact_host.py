"""The bit-exact restatement of the layer-wise train path (tests/train_exact_restatement.py) checked on the CPU, before
tests/test_gpu_train_edges.py holds the kernels to it:

* fma32 against libm's fmaf (ctypes, nothing compiled), on random operands and on operands built from bit patterns for which
  "float64, then cast" rounds twice and lands on the wrong f32;
* the exact forward and backward against float64, layer by layer, within the bound of an n-operation chain, (n + 4) 2^-24 sum |terms|
  (n fmas or adds, each with a relative rounding error of at most 2^-24; the second-order terms are covered by the margin of 4);
* the sparse-upstream property the GPU tests rest on: with an upstream gradient that is zero outside some points, the backward over
  those points' rows alone equals the backward over all rows byte for byte;
* the column-sum order against a direct statement of "lane j takes blocks j, j + 8, ...".

A narrow decoder (hidden width 32, C = 5) keeps it quick: the restatement reads every width from the weights.
"""
import ctypes

import numpy as np
import pytest

import train_exact_restatement as ex
import train_restatement as tr

U = 2.0 ** -24
F32 = np.float32
COUNTS = [1, 65, 0, 63, 64]          # 320 rows: two K slabs (256 + 64) with the cut inside a segment, one empty segment


def _libm_fmaf():
    f = ctypes.CDLL('libm.so.6').fmaf
    f.restype, f.argtypes = ctypes.c_float, [ctypes.c_float] * 3
    return f


def test_fma32_is_fmaf_on_random_operands():
    fmaf = _libm_fmaf()
    rs = np.random.RandomState(1)
    n = 40000
    a = (rs.standard_normal(n) * 2.0 ** rs.randint(-20, 20, n)).astype(F32)
    b = (rs.standard_normal(n) * 2.0 ** rs.randint(-20, 20, n)).astype(F32)
    c = (rs.standard_normal(n) * 2.0 ** rs.randint(-30, 30, n)).astype(F32)
    c[::3] = (-(a[::3].astype(np.float64) * b[::3].astype(np.float64))).astype(F32)         # cancellation: the result is the product's tail
    c[1::7] = 0
    got = ex.fma32(a, b, c)
    ref = np.array([fmaf(float(x), float(y), float(z)) for x, y, z in zip(a, b, c)], F32)
    assert got.tobytes() == ref.tobytes()


def test_fma32_where_float64_then_cast_rounds_twice():
    """c = m 2^(e+1) with a 24-bit m, and a b = -+(1 - i^2 2^-46) 2^e from a = (1 + i 2^-23) 2^e, b = -+(1 - i 2^-23): the exact sum sits
    i^2 2^(e-46) beside the f32 midpoint (m -+ 1/2) 2^(e+1), float64 (53 bits) rounds it onto the midpoint, and the cast then ties to
    even -- the wrong side whenever m's neighbour on that side is even."""
    fmaf = _libm_fmaf()
    rs = np.random.RandomState(2)
    n = 4000
    m = rs.randint(1 << 23, 1 << 24, n).astype(np.int64)
    i = rs.randint(1, 200, n).astype(np.int64)
    e = rs.randint(-30, 30, n)
    sign = np.where(rs.rand(n) < 0.5, -1.0, 1.0)
    c_sign = np.where(rs.rand(n) < 0.5, -1.0, 1.0)
    a = ((1 << 23) + i).astype(np.float64) * 2.0 ** (e - 23)
    b = sign * ((1 << 24) - 2 * i).astype(np.float64) * 2.0 ** -24
    c = c_sign * m.astype(np.float64) * 2.0 ** (e + 1)
    a32, b32, c32 = a.astype(F32), b.astype(F32), c.astype(F32)
    assert (a32 == a).all() and (b32 == b).all() and (c32 == c).all()                      # every operand is an f32 value
    got = ex.fma32(a32, b32, c32)
    ref = np.array([fmaf(float(x), float(y), float(z)) for x, y, z in zip(a32, b32, c32)], F32)
    naive = (a * b + c).astype(F32)
    twice = int((naive != ref).sum())
    print('%d of %d constructed cases: float64-then-cast differs from fmaf' % (twice, n))
    assert twice >= n // 4
    assert got.tobytes() == ref.tobytes()


def narrow_decoder(seed=5, H=32, Cn=5):
    rs = np.random.RandomState(seed)
    n3 = H - 3 - Cn
    shapes = [(H, Cn + 3), (H, H), (H, H), (n3, H), (H, H), (H, H), (H, H), (H, H), (1, H)]
    Ws = [(rs.standard_normal(s) * np.sqrt(2.0 / s[1])).astype(F32) for s in shapes]
    bs = [(0.1 * rs.standard_normal(s[0])).astype(F32) for s in shapes]
    return Ws, bs


@pytest.fixture(scope='module')
def small():
    Ws, bs = narrow_decoder()
    rs = np.random.RandomState(6)
    n = sum(COUNTS)
    codes = rs.standard_normal((len(COUNTS), 5)).astype(F32)
    pts = ((rs.rand(n, 3) - 0.5) * 1.6).astype(F32)
    seg, idx, pt = ex.row_table(COUNTS)
    xyz = np.where(pt[:, None] >= 0, pts[np.maximum(pt, 0)], F32(0)).astype(F32)
    return dict(Ws=Ws, bs=bs, codes=codes, pts=pts, seg=seg, idx=idx, pt=pt, xyz=xyz, rows=np.arange(len(seg)))


DROPOUTS = [None, ((0, 3, 7), 0.5, 77, 3), (tuple(range(8)), 0.2, 78, 0)]


def _dropout(spec):
    import dropout_restatement as dr
    if spec is None:
        return None
    layers, p, seed, base = spec
    return (layers, dr.threshold(p), dr.scale(p), seed, base)


def _chain_bound(n_ops, S):
    return (n_ops + 4) * U * S


@pytest.mark.parametrize('spec', DROPOUTS)
def test_exact_chains_against_float64(small, spec):
    """Layer-local: every exact f32 result against float64 arithmetic on the SAME f32 inputs, within the chain bound."""
    c, drop = small, _dropout(spec)
    Ws, bs = c['Ws'], c['bs']
    H, n3, Cn = ex.widths(Ws)
    W64, b64 = [W.astype(np.float64) for W in Ws], [b.astype(np.float64) for b in bs]
    X, z = ex.forward_rows(Ws, bs, c['codes'], c['seg'], c['idx'], c['xyz'], drop)
    scale = 1.0 if drop is None else float(drop[2])
    inp = np.concatenate([c['codes'][c['seg']], c['xyz']], 1).astype(np.float64)
    x = inp
    for l in range(9):
        if l == 4:
            x = np.concatenate([x, inp], 1)
        pre = x @ W64[l].T + b64[l]
        S = np.abs(x) @ np.abs(W64[l]).T + np.abs(b64[l])
        n_ops = x.shape[1] + 1                      # (+ 1: the dropout's multiply)
        if l == 8:
            assert (np.abs(z - pre[:, 0]) <= _chain_bound(n_ops, S[:, 0])).all()
            break
        got = X[l + 1].astype(np.float64)
        live = got != 0
        f = scale if drop is not None and l in drop[0] else 1.0
        assert (np.abs(got - f * pre)[live] <= _chain_bound(n_ops, f * S)[live]).all(), l
        if f == 1.0:
            assert (pre[~live] <= _chain_bound(n_ops, S)[~live]).all(), l
        else:
            big = pre > _chain_bound(n_ops, S)
            assert (big & ~live).any() and (big & live).any(), l                           # the mask drops some units and keeps some
        x = got                                      # the next layer reads the f32 values
    # the backward, from a dz on every real row
    rs = np.random.RandomState(9)
    dz = np.where(c['pt'] >= 0, rs.standard_normal(len(c['pt'])), 0).astype(F32)
    g_W, g_b, g_lat, deltas = ex.backward_rows(Ws, c['codes'], COUNTS, c['rows'], c['xyz'], X, dz, drop)
    P = len(dz)
    for l in range(8, 0, -1):
        N = n3 if l == 4 else H
        d_out = deltas[l].astype(np.float64)
        f = scale if drop is not None and (l - 1) in drop[0] else 1.0
        gate = (X[l][:, :N] > 0) * f
        ref = (d_out @ W64[l][:, :N]) * gate
        S = (np.abs(d_out) @ np.abs(W64[l][:, :N])) * gate
        assert (np.abs(deltas[l - 1] - ref) <= _chain_bound(d_out.shape[1] + 1, S)).all(), l
    for m in range(9):
        d = deltas[m].astype(np.float64)
        n_ops = P + 8                                # rows, then the slabs / the lanes and their tree / the segments
        assert (np.abs(g_b[m] - d.sum(0)) <= _chain_bound(n_ops, np.abs(d).sum(0))).all(), m
        if m >= 1:
            K = n3 if m == 4 else H
            xm = X[m][:, :K].astype(np.float64)
            assert (np.abs(g_W[m][:, :K] - d.T @ xm) <= _chain_bound(n_ops, np.abs(d).T @ np.abs(xm))).all(), m
        if m in (0, 4):
            lat0 = 0 if m == 0 else n3
            refl, refx = d.T @ inp[:, :Cn], d.T @ inp[:, Cn:]
            Sl, Sx = np.abs(d).T @ np.abs(inp[:, :Cn]), np.abs(d).T @ np.abs(inp[:, Cn:])
            assert (np.abs(g_W[m][:, lat0:lat0 + Cn] - refl) <= _chain_bound(n_ops + len(COUNTS), Sl)).all(), m
            assert (np.abs(g_W[m][:, lat0 + Cn:] - refx) <= _chain_bound(n_ops, Sx)).all(), m
    for s in range(len(COUNTS)):
        at = c['seg'] == s
        d0, d4 = deltas[0][at].astype(np.float64), deltas[4][at].astype(np.float64)
        ref = d0.sum(0) @ W64[0][:, :Cn] + d4.sum(0) @ W64[4][:, n3:n3 + Cn]
        S = np.abs(d0).sum(0) @ np.abs(W64[0][:, :Cn]) + np.abs(d4).sum(0) @ np.abs(W64[4][:, n3:n3 + Cn])
        assert (np.abs(g_lat[s] - ref) <= _chain_bound(2 * H + 64 + 8, S)).all(), s
    assert not g_lat[2].any()


def test_exact_run_against_the_float64_restatement(small):
    """End to end, no dropout: sdf and every gradient against tests/train_restatement.py with the exact run's gates, at the project's
    bars (2e-6 on tanh z; 1e-4 of a tensor's largest entry)."""
    c = small
    X, z = ex.forward_rows(c['Ws'], c['bs'], c['codes'], c['seg'], c['idx'], c['xyz'])
    real = c['pt'] >= 0
    import torch
    gates = [torch.from_numpy(X[l + 1][real] > 0) for l in range(8)]
    rs = np.random.RandomState(10)
    w = rs.standard_normal(sum(COUNTS)).astype(F32)
    y, _, ref_W, ref_b, ref_rows = tr.gradients(c['Ws'], c['bs'], c['codes'], c['pts'], COUNTS, w, None, gates=gates)
    s = np.tanh(z.astype(np.float64))
    assert np.abs(s[real] - y.numpy()[:, 0]).max() <= 2e-6
    dz = np.zeros(len(z), F32)
    dz[real] = (w.astype(np.float64) * (1 - s[real] ** 2)).astype(F32)
    g_W, g_b, g_lat, _ = ex.backward_rows(c['Ws'], c['codes'], COUNTS, c['rows'], c['xyz'], X, dz)
    for l in range(9):
        for got, ref in ((g_W[l], ref_W[l].numpy()), (g_b[l], ref_b[l].numpy())):
            assert got.shape == ref.shape and np.abs(got - ref).max() <= 1e-4 * np.abs(ref).max(), l
    for s_ in range(len(COUNTS)):
        assert np.abs(g_lat[s_] - ref_rows[s_].numpy()).max() <= 1e-4 * max(np.abs(ref_rows[s_].numpy()).max(), 1e-30), s_


@pytest.mark.parametrize('spec', DROPOUTS[:2])
def test_sparse_upstream_needs_the_probe_rows_only(small, spec):
    c, drop = small, _dropout(spec)
    seg_row = ex.train_segment_rows(COUNTS)
    probes = [0, 64, 127, 128, 192, 254, 256, 319]     # first / last points, in-segment 63 / 64, either side of the slab cut at row 256
    assert all(c['pt'][r] >= 0 for r in probes) and seg_row == [0, 64, 192, 192, 256, 320]
    X, _ = ex.forward_rows(c['Ws'], c['bs'], c['codes'], c['seg'], c['idx'], c['xyz'], drop)
    rs = np.random.RandomState(11)
    dz = np.zeros(len(c['pt']), F32)
    dz[probes] = rs.standard_normal(len(probes)).astype(F32)
    full = ex.backward_rows(c['Ws'], c['codes'], COUNTS, c['rows'], c['xyz'], X, dz, drop)
    Xp = [None] + [x[probes] for x in X[1:]]
    part = ex.backward_rows(c['Ws'], c['codes'], COUNTS, probes, c['xyz'][probes], Xp, dz[probes], drop)
    for l in range(9):
        assert ex.same_bytes(full[0][l], part[0][l]) and ex.same_bytes(full[1][l], part[1][l]), l
        assert full[0][l].any()
    assert ex.same_bytes(full[2], part[2]) and not full[2][2].any() and full[2][0].any()
    # and the rows outside the probes carry exact zeros
    rest = np.setdiff1d(c['rows'], probes)
    assert all(not full[3][l][rest].any() for l in range(9))


@pytest.mark.parametrize('nb', [1, 8, 9, 17])
def test_column_sum_order(nb):
    """Lane j adds blocks j, j + 8, ... in order, starting from 0; then ((0+1)+(2+3))+((4+5)+(6+7)). The values are spread over many
    binades, so that another order gives other bytes."""
    rs = np.random.RandomState(20 + nb)
    part = (rs.standard_normal((nb, 64)) * 2.0 ** rs.randint(-12, 12, (nb, 64))).astype(F32)
    lanes = []
    for j in range(8):
        a = np.zeros(64, F32)
        for b in [b for b in range(nb) if b % 8 == j]:
            a = (a + part[b]).astype(F32)
        lanes.append(a)
    p01, p23, p45, p67 = lanes[0] + lanes[1], lanes[2] + lanes[3], lanes[4] + lanes[5], lanes[6] + lanes[7]
    ref = (p01 + p23) + (p45 + p67)
    got = ex.column_sum_order(part)
    assert got.dtype == F32 and got.tobytes() == ref.astype(F32).tobytes()
    if nb > 8:
        serial = np.zeros(64, F32)
        for b in range(nb):
            serial = serial + part[b]
        assert serial.tobytes() != got.tobytes()
