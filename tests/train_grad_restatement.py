"""Float64 numpy restatement of the spatial gradient g = grad_x f of the DeepSDF 8x512 decoder (latent_in=[4]) and of the gradients of a
loss L(f, g) to the eighteen weight tensors and the codes, written from the closed form -- no autograd:

    in_0 = [code | xyz], in_4 = [X_4 | code | xyz], in_l = X_l otherwise;  X_(l+1) = G_l (W_l in_l + b_l),  G_l = scale_l [gate_l]
    z = W_8 X_8 + b_8, f = tanh z, t' = 1 - f^2
    unit deltas   Delta_8 = 1, Delta_(l-1) = G_(l-1) (Delta_l W_l[:, activation columns])
    forward       g = t' (Delta_0 W0[:, xyz] + Delta_4 W4[:, xyz])
    tangent       tau_0 = [0 | u], tau_(l+1) = G_l (W_l tau_l) with tau_4's input [tau_4 | 0 | u], Q = W_8 tau_8
    row scalars   c1 = t', c2 = t' (phi - 2 f Q)                              (phi = dL/df, u = dL/dg)
    gradients     g_W_l = sum_rows Delta_l (x) (c2 in_l + c1 tau_l),  g_b_l = sum_rows c2 Delta_l,
                  g_code_s = W0[:, code]^T sum_(rows of s) c2 Delta_0 + W4[:, code]^T sum_(rows of s) c2 Delta_4

The ReLU's second derivative is zero. gate_l is the ReLU pattern of the restatement's own pre-activations, or GIVEN (the pattern a GPU run
saved, as in tests/train_restatement.py: then both differentiate the same piecewise-linear function), and with `keeps` also the dropout
keep; scale_l is the dropout factor of a dropped layer, 1 elsewhere. tests/test_train_grad_host.py pins this file to float64
torch.autograd double backward through the project's Decoder.
"""
import numpy as np


def _f64(a):
    return np.asarray(a.detach().cpu() if hasattr(a, 'detach') else a, dtype=np.float64)


def restate(Ws, bs, codes, pts, counts, phi, u, gates=None, keeps=None, scale=1.0):
    """Ws, bs: nine arrays each; codes (S, C) or (1, C) shared; pts (n, 3), n = sum counts; phi (n,) or (n, 1) or None; u (n, 3) or None.
    gates: None or eight bool arrays, gates[l] of lin_l's output shape; keeps: None or eight entries, each None (layer not dropped) or a
    bool array of lin_l's output shape; scale: the factor of a kept unit in a dropped layer.
    -> dict(f (n, 1), g (n, 3), g_W [9], g_b [9], g_codes (S, C) one row per segment, gates [8] as used)"""
    Ws, bs = [_f64(W) for W in Ws], [_f64(b) for b in bs]
    codes, pts = _f64(codes), _f64(pts).reshape(-1, 3)
    counts = [int(c) for c in counts]
    n, S = pts.shape[0], len(counts)
    C, n3, ld4 = Ws[0].shape[1] - 3, Ws[3].shape[0], Ws[4].shape[1]
    assert n == sum(counts) and ld4 == n3 + C + 3
    phi = np.zeros(n) if phi is None else _f64(phi).reshape(n)
    u = np.zeros((n, 3)) if u is None else _f64(u).reshape(n, 3)
    seg = np.repeat(np.arange(S), counts)
    rows = (np.repeat(codes, S, 0) if codes.shape[0] == 1 else codes)[seg]
    in0 = np.concatenate([rows, pts], 1)

    # forward, with the gate G_l of every layer
    G, ins, used = [], [], []
    x = in0
    for l in range(8):
        if l == 4:
            x = np.concatenate([x, in0], 1)
        ins.append(x)
        zl = x @ Ws[l].T + bs[l]
        gate = (zl > 0) if gates is None else np.asarray(gates[l].cpu() if hasattr(gates[l], 'cpu') else gates[l]).astype(bool)
        sc = 1.0
        if keeps is not None and keeps[l] is not None:
            gate = gate & np.asarray(keeps[l]).astype(bool)
            sc = float(scale)
        used.append(gate)
        G.append(sc * gate)
        x = G[l] * zl
    ins.append(x)
    f = np.tanh(x @ Ws[8].T + bs[8])                    # (n, 1)
    tp = 1.0 - f * f

    # unit deltas
    D = [None] * 9
    D[8] = np.ones((n, 1))
    for l in range(8, 0, -1):
        Wl = Ws[l][:, :n3] if l == 4 else Ws[l]
        D[l - 1] = G[l - 1] * (D[l] @ Wl)
    g = tp * (D[0] @ Ws[0][:, C:C + 3] + D[4] @ Ws[4][:, ld4 - 3:])

    # tangent along u
    zeros = np.zeros((n, C))
    tau0 = np.concatenate([zeros, u], 1)
    taus, t = [], tau0
    for l in range(8):
        if l == 4:
            t = np.concatenate([t, tau0], 1)
        taus.append(t)
        t = G[l] * (t @ Ws[l].T)
    taus.append(t)
    Q = t @ Ws[8].T                                     # (n, 1)

    c1 = tp
    c2 = tp * (phi[:, None] - 2.0 * f * Q)
    g_W = [D[l].T @ (c2 * ins[l] + c1 * taus[l]) for l in range(9)]
    g_b = [(c2 * D[l]).sum(0) for l in range(9)]
    g_codes = np.zeros((S, C))
    for s in range(S):
        m = seg == s
        g_codes[s] = (c2[m] * D[0][m]).sum(0) @ Ws[0][:, :C] + (c2[m] * D[4][m]).sum(0) @ Ws[4][:, n3:n3 + C]
    return dict(f=f, g=g, g_W=g_W, g_b=g_b, g_codes=g_codes, gates=used)
