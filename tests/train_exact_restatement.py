"""Bit-exact f32 restatement of the layer-wise train path (DESIGN.md sections 8f and 8g), in numpy, written from the document's statement
of every sum's order -- not from the kernels. It works on a handful of workspace rows (the "probe rows"): the forward is row-independent,
and with an upstream gradient that is non-zero at the probe points only every other row's deltas are exact zeros, which add exactly
nothing to a fmaf chain or to a plain f32 sum; so the probe rows alone give every gradient byte for byte.

fma32 is an exact fmaf without a compiler: the float64 product of two f32 values is exact; the float64 sum with the addend is rounded
to odd (TwoSum error term; one step towards the error when the sum is inexact and its last bit even), which makes the final rounding to
f32 the rounding of the exact value (53 >= 24 + 2 bits).

The widths are read from the weights (hidden width = W1's rows, lin3's outputs = W3's rows, C = W0's columns - 3), so the host tests
can run a narrow decoder; the library's is 512 wide.
"""
import numpy as np

import dropout_restatement as dr
from distr.functions import TRAIN_ROW_TILE, train_segment_rows, train_slab_plan

F32, F64 = np.float32, np.float64


def fma32(a, b, c):
    """round_f32(a * b + c) with one rounding, for f32 arrays (broadcast against each other)."""
    a, b, c = np.asarray(a, F32), np.asarray(b, F32), np.asarray(c, F32)
    return _fma_p(a.astype(F64) * b.astype(F64), c.astype(F64))


def _fma_p(p, c):
    """p: an exact float64 product of two f32 values, c: an f32 value held in float64 -> f32 of the exact p + c."""
    p, c = np.broadcast_arrays(p, c)
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)                      # TwoSum: p + c = s + e exactly
    fix = (e != 0) & ((np.ascontiguousarray(s).view(np.int64) & 1) == 0)
    if fix.any():
        s = np.where(fix, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
    return s.astype(F32)


def chain(acc, A, B):
    """acc = fmaf(A[k], B[k], acc) for k in order; A[k] and B[k] broadcast against acc's shape. Returns f32."""
    A64, B64 = np.asarray(A, F32).astype(F64), np.asarray(B, F32).astype(F64)
    acc = np.asarray(acc, F32)
    for k in range(A64.shape[0]):
        acc = _fma_p(A64[k] * B64[k], acc.astype(F64))
    return acc


def widths(Ws):
    """(hidden width H, lin3's outputs = lin4's activation columns, C)"""
    return Ws[1].shape[0], Ws[3].shape[0], Ws[0].shape[1] - 3


def row_table(counts):
    """Per workspace row of the padded list: (segment, index inside the segment, point index in the caller's list or -1)."""
    seg, idx, pt, p0 = [], [], [], 0
    for s, n in enumerate(counts):
        pad = -(-int(n) // TRAIN_ROW_TILE) * TRAIN_ROW_TILE
        seg += [s] * pad
        idx += list(range(pad))
        pt += [p0 + i if i < n else -1 for i in range(pad)]
        p0 += int(n)
    return np.array(seg, np.int64), np.array(idx, np.int64), np.array(pt, np.int64)


def _relu(v):
    return np.where(v > 0, v, F32(0))


def _drop(X, layer, seg, idx, dropout):
    """dropout = None or (layers, threshold, scale, seed, segment_base): v * scale (one f32 multiply) or +0 behind the relu."""
    if dropout is None or layer not in dropout[0]:
        return X
    _, T, scale, seed, base = dropout
    keep = dr.keep_at(seed, T, layer, (base + seg)[:, None], idx[:, None], np.arange(X.shape[1])[None, :])
    return np.where(keep, X * F32(scale), F32(0)).astype(F32)


def forward_rows(Ws, bs, codes, seg, idx, xyz, dropout=None):
    """The forward on given workspace rows. seg, idx (P,): each row's segment and index inside it; xyz (P, 3) f32, zeros for a padded row;
    codes (S, C) or (1, C) shared. Returns ([None, X_1 .. X_8], z (P,)): X_l (P, H) f32, X_4 with lin3's columns only."""
    Ws, bs = [np.asarray(W, F32) for W in Ws], [np.asarray(b, F32) for b in bs]
    H, n3, C = widths(Ws)
    codes, xyz = np.asarray(codes, F32), np.asarray(xyz, F32)
    cs = np.zeros(len(seg), np.int64) if codes.shape[0] == 1 else seg
    used = sorted(set(int(s) for s in cs))
    c0, c4 = {}, {}
    for s in used:
        c0[s] = chain(bs[0], Ws[0][:, :C].T, codes[s][:, None])
        c4[s] = chain(bs[4], Ws[4][:, n3:n3 + C].T, codes[s][:, None])
    a = np.stack([c0[int(s)] for s in cs])
    for d in range(3):
        a = fma32(Ws[0][:, C + d][None, :], xyz[:, d:d + 1], a)
    X = [None, _drop(_relu(a), 0, seg, idx, dropout)]
    for l in range(1, 8):
        K = n3 if l == 4 else H
        start = np.stack([c4[int(s)] for s in cs]) if l == 4 else np.broadcast_to(bs[l], (len(seg), Ws[l].shape[0]))
        a = chain(start, X[l][:, :K].T[:, :, None], Ws[l][:, :K].T[:, None, :])
        if l == 4:
            for d in range(3):
                a = fma32(Ws[4][:, n3 + C + d][None, :], xyz[:, d:d + 1], a)
        X.append(_drop(_relu(a), l, seg, idx, dropout))
    z = chain(np.broadcast_to(bs[8], (len(seg), 1)), X[8].T[:, :, None], Ws[8].T[:, None, :])[:, 0]
    return X, z


def column_sum_order(part):
    """part (nb, ...) f32, the block sums of one segment's nb blocks -> the segment's sum: eight partial sums, lane j over blocks
    j, j + 8, ... in block order from 0, then ((0+1)+(2+3))+((4+5)+(6+7))."""
    part = np.asarray(part, F32)
    lane = []
    for j in range(8):
        a = np.zeros(part.shape[1:], F32)
        for b in range(j, part.shape[0], 8):
            a = a + part[b]
        lane.append(a)
    return ((lane[0] + lane[1]) + (lane[2] + lane[3])) + ((lane[4] + lane[5]) + (lane[6] + lane[7]))


def _segment_sums(delta, rows, xyz, counts, moments):
    """(S, 4, n) f32: per segment the sum of delta's columns (q = 0) and, with moments, of delta * x / y / z (q = 1..3, per-row fmas).
    Rows in row order inside a 64-row block from 0, blocks as column_sum_order says. Rows not given are exact zeros."""
    seg_row = train_segment_rows(counts)
    n = delta.shape[1]
    part = np.zeros((seg_row[-1] // TRAIN_ROW_TILE, 4, n), F32)
    for i, r in enumerate(rows):
        b = int(r) // TRAIN_ROW_TILE
        part[b, 0] = part[b, 0] + delta[i]
        if moments:
            for d in range(3):
                part[b, 1 + d] = fma32(delta[i], xyz[i, d], part[b, 1 + d])
    return np.stack([column_sum_order(part[seg_row[s] // TRAIN_ROW_TILE: seg_row[s + 1] // TRAIN_ROW_TILE]) for s in range(len(counts))])


def _weight_grad(delta, Xm, rows, total_rows):
    """(M, N) f32 = delta^T Xm: per K slab a chain over the slab's rows in row order from 0, the slabs added in slab order starting
    from slab 0's value. Rows not given are exact zeros."""
    L, nslab = train_slab_plan(total_rows)
    slab = np.asarray(rows) // L
    total = None
    for z in range(nslab):
        at = np.nonzero(slab == z)[0]
        if z > 0 and len(at) == 0:
            continue                                    # + 0: exact
        part = chain(np.zeros((delta.shape[1], Xm.shape[1]), F32), delta[at][:, :, None], Xm[at][:, None, :])
        total = part if total is None else total + part
    return total


def backward_rows(Ws, codes, counts, rows, xyz, X, dz, dropout=None):
    """The backward from the given rows' dz (every other row's dz is zero). rows: sorted workspace rows; xyz (P, 3); X: forward_rows'
    list on the same rows; dz (P,) f32. Returns (g_W [9], g_b [9], g_latent (S, C), deltas {l: (P, out_l)})."""
    Ws = [np.asarray(W, F32) for W in Ws]
    H, n3, C = widths(Ws)
    codes = np.asarray(codes, F32)
    S = len(counts)
    code_of = (lambda s: codes[0]) if codes.shape[0] == 1 else (lambda s: codes[s])
    rows = np.asarray(rows, np.int64)
    assert (np.diff(rows) > 0).all()
    R = train_segment_rows(counts)[-1]
    drop_layers, scale = (dropout[0], F32(dropout[2])) if dropout is not None else ((), F32(1))
    g_W, g_b, deltas, segsum = [None] * 9, [None] * 9, {}, {}

    def bias_and_columns(m, delta):
        ss = _segment_sums(delta, rows, xyz, counts, m in (0, 4))
        segsum[m] = ss
        b = np.zeros(delta.shape[1], F32)
        for s in range(S):
            b = b + ss[s, 0]
        g_b[m] = b
        if m in (0, 4):
            lat = np.zeros((delta.shape[1], C), F32)
            for s in range(S):
                lat = fma32(ss[s, 0][:, None], code_of(s)[None, :], lat)
            mom = np.zeros((delta.shape[1], 3), F32)
            for s in range(S):
                mom = mom + ss[s, 1:4].T
            return lat, mom

    delta = np.asarray(dz, F32)[:, None]
    deltas[8] = delta
    g_W[8] = _weight_grad(delta, X[8], rows, R)
    bias_and_columns(8, delta)
    for l in range(8, 0, -1):
        N = n3 if l == 4 else H
        d = chain(np.zeros((len(rows), N), F32), delta.T[:, :, None], Ws[l][:, :N][:, None, :])
        gate = X[l][:, :N] > 0
        delta = np.where(gate, d * scale if (l - 1) in drop_layers else d, F32(0)).astype(F32)
        m = l - 1
        deltas[m] = delta
        if m >= 1:
            K = n3 if m == 4 else H
            act = _weight_grad(delta, X[m][:, :K], rows, R)
            if m == 4:
                lat, mom = bias_and_columns(4, delta)
                g_W[4] = np.concatenate([act, lat, mom], 1)
            else:
                g_W[m] = act
                bias_and_columns(m, delta)
        else:
            lat, mom = bias_and_columns(0, delta)
            g_W[0] = np.concatenate([lat, mom], 1)
    g_lat = np.zeros((S, C), F32)
    for s in range(S):
        a = chain(np.zeros(C, F32), Ws[0][:, :C], segsum[0][s, 0][:, None])
        g_lat[s] = chain(a, Ws[4][:, n3:n3 + C], segsum[4][s, 0][:, None])
    return g_W, g_b, g_lat, deltas


def same_bytes(a, b):
    """Byte equality of two f32 arrays, with +0 and -0 counted as equal (and no NaN on either side)."""
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype == F32 and a.shape == b.shape and bool(np.array_equal(a, b))
