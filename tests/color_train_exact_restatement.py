"""Bit-exact f32 restatement of the layer-wise train path on a DESCRIBED network: what
tests/train_exact_restatement.py restates for one output column, for lin8 with several rows. Written from the document's statement of the
sums' orders, out of that module's pieces (fma32, chain, the segment sums, the slab order) -- it reads every width from the weights
(lin3's outputs = W3's rows, the code length = W0's columns - 3, so lin4's columns are [lin3 outputs | code | xyz] at any row stride),
and only the output side is new here:

  z[row][ch]      = the k-ordered chain from b8[ch] over X_8[row][k] W8[ch][k]                         (lin8 as a GEMM with nout columns)
  delta_8         = dz (P, nout); g_W8 = delta_8^T X_8 in slab order; g_b8[ch] = the ordered column sums of dz[:, ch]
  delta_7[row][n] = the chain over ch = 0 .. nout - 1 of dz[row][ch] W8[ch][n], gated by X_8 > 0
"""
import numpy as np

import train_exact_restatement as ex
from train_exact_restatement import F32, chain, fma32, row_table, same_bytes, train_segment_rows, widths  # noqa: F401


def forward_rows(Ws, bs, codes, seg, idx, xyz, dropout=None):
    """([None, X_1 .. X_8], z (P, nout)) on the given workspace rows; X_4 with lin3's columns only."""
    Ws, bs = [np.asarray(W, F32) for W in Ws], [np.asarray(b, F32) for b in bs]
    X, _ = ex.forward_rows(Ws[:8] + [Ws[8][:1]], bs[:8] + [bs[8][:1]], codes, seg, idx, xyz, dropout)
    z = chain(np.broadcast_to(bs[8], (len(seg), Ws[8].shape[0])), X[8].T[:, :, None], Ws[8].T[:, None, :])
    return X, z


def backward_rows(Ws, codes, counts, rows, xyz, X, dz, dropout=None):
    """The backward from the given rows' dz (P, nout); every other row's dz is zero. Returns (g_W [9], g_b [9], g_latent (S, L))."""
    Ws = [np.asarray(W, F32) for W in Ws]
    H, n3, C = widths(Ws)
    codes = np.asarray(codes, F32)
    S = len(counts)
    code_of = (lambda s: codes[0]) if codes.shape[0] == 1 else (lambda s: codes[s])
    rows = np.asarray(rows, np.int64)
    assert (np.diff(rows) > 0).all()
    R = train_segment_rows(counts)[-1]
    drop_layers, scale = (dropout[0], F32(dropout[2])) if dropout is not None else ((), F32(1))
    g_W, g_b, segsum = [None] * 9, [None] * 9, {}

    def bias_and_columns(m, delta):
        ss = ex._segment_sums(delta, rows, xyz, counts, m in (0, 4))
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

    delta = np.asarray(dz, F32).reshape(len(rows), Ws[8].shape[0])
    g_W[8] = ex._weight_grad(delta, X[8], rows, R)
    bias_and_columns(8, delta)
    for l in range(8, 0, -1):
        N = n3 if l == 4 else H
        d = chain(np.zeros((len(rows), N), F32), delta.T[:, :, None], Ws[l][:, :N][:, None, :])
        delta = np.where(X[l][:, :N] > 0, d * scale if (l - 1) in drop_layers else d, F32(0)).astype(F32)
        m = l - 1
        if m >= 1:
            act = ex._weight_grad(delta, X[m][:, :(n3 if m == 4 else H)], rows, R)
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
    return g_W, g_b, g_lat
