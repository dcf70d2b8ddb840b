"""A plain restatement of the fused losses (csrc/distr_losses.hpp): f3, the single-view losses (k_single_loss_partial / _final / _bwd) and f2,
the warp loss (k_warp_fwd / _final / _bwd, k_sum_partials). CPU only, numpy, float64 unless the caller asks for another type.

Every input enters as the float32 (uint8) value the kernels see and is widened here; nothing is rounded. With dtype=np.float32 the same text
runs in float32 (tests/test_losses_edges_host.py: what a plain float32 evaluation of the closed forms gives).

Each output comes with the magnitude its bar is measured against: for a per-pixel gradient entry the sum of the absolute values of the
float64 terms that form it; for a loss or a camera sum, A = the sum of that quantity over the contributing pixels (divided like the loss).
A bar is k 2^-24 A, k = the float32 roundings on the longest path to the output, counted from the kernels: one per float32
multiplication, addition, division and square root (the library is built without contraction). An operand's roundings add in a product
or quotient; a sum carries the larger count of its terms plus one.

f3, per pixel term                                     roundings
  hinges   q - t, t - q                                 1
  depth    d - gd                                       1
  normal   nn = sqrt(n0 n0 + n1 n1 + n2 n2)             mul, add, add, sqrt            4
           e = nn + 1e-12                                                                5
           n_a / e                                      1 + 5                            6
           bh_a = b_a / (|b| + 1e-12)                   the same                         6
           (n_a / e) bh_a                               6 + 6 + 1                       13
           the sum of three                             add, add                        15
  reduction (block_sum, k_single_loss_final)            6 shuffle levels + 3 wave adds + nblk ordered partials + the division
  -> K_LOSS = {hinge 1, depth 1, normal 15} + 10 + nblk
f3, gradients (k_single_loss_bwd)
  g_min_sdf, g_depth   g / count                        1
  g_normal_a = -w (bh_a / e - nb n_a / (nn e e))
           w = g / count                                1
           bh_a / e                                     6 + 5 + 1                       12
           nb = sum n_b bh_b                            6 + 1, add, add                  9
           nb n_a                                                                       10
           nn e e                                       4 + 5 + 1, + 5 + 1              16
           the quotient                                 10 + 16 + 1                     27
           the difference                                                               28
           times w                                      28 + 1 + 1                      30

f2, per valid pixel (warp_pixel), counted against the magnitudes below
  h = K_inv (x, y, 1) 3 | r = R1^T h 6 | rn 10 | e 11 | d = r / e 18 | c1 = -R1^T T1 3 | pt = d z + c1 20 | q = R2 pt + T2 24
  pr = K q 27 | u = pr0 / pr2 55 | gx = 2 u / (W - 1) - 1 57 | ix = ((gx + 1) / 2) (W - 1) 59 | tx = ix - floor(ix) 60      K_COORD = 60
  The coordinate's roundings are relative to Mx = |u| + (W - 1), not to tx: one of them moves tx by 2^-24 Mx. What depends on (tx, ty)
  therefore carries a sensitivity term in its magnitude: |d . / d ix| Mx + |d . / d iy| My.
  d2     calib 12, wgt 3, z2 calib wgt 17, four corners 21; err = pr2 - d2; err err                 K_D2 = 21, K_PR = 27
  c2     wgt 3, img2 wgt 4, four corners 8                                                           K_C2 = 8
  c2 depends on (tx, ty): its roundings are counted as the coordinate's 60 against c2_A = sum |img2 wgt| + |d c2 / d ix| Mx + |d c2 / d iy| My
  loss   c1 - c2 61 (against |c1| + c2_A), three channels 63, the reduction 6 + 3 + nblk, times 3, the division     63 + 9 + nblk + 2
f2, gradients. k_warp_bwd forms a pixel's 24 camera terms and its g_z1 in float64 from the float32 inputs and rounds each ONCE
(as k_samp_cam_bwd does), so a pixel's entry has 1 rounding, and a camera sum 1 + 6 + 3 + nblk:                K_CAM = 10 + nblk
  A of a camera entry is the sum over the kept pixels of the absolute value of the pixel's finished float64 term.
  The float32 evaluation the kernel did before is counted in `K_F32` (host test): gc 2, gix 9 + the coordinate 60, gpr 145, gq 148,
  g_R2 169, gpt 151, g_z 172, g_d 152, the ray part 208, g_R1 210, g_T1 155; against A it fails for single pixels.

Rules float64 cannot decide are written as the kernel writes them, each with the reference line it restates.
"""
import numpy as np

EPS = float(np.float32(1e-12))       # the kernels' 1e-12f
U = 2.0 ** -24
K_TERM = (1, 1, 1, 15)               # mask_gt, mask_out, depth, normal
K_GRAD = dict(min_sdf=1, depth=1, normal=30)
K_COORD, K_D2, K_PR, K_C2 = 60, 21, 27, 8
K_F32 = dict(g_z=172, g_R1=210, g_T1=155, g_R2=169, g_T2=148)


def nblk(P):
    return (int(P) + 255) // 256


def k_single_loss(term, P):
    """per-term roundings + 6 shuffle levels + 3 wave adds + nblk ordered partials + the division."""
    return K_TERM[term] + 6 + 3 + nblk(P) + 1


def k_warp_loss(P):
    """c2 (the coordinate's 60, against c2_A) + the difference + three channels (2) + 6 + 3 + nblk + 3 * kept + the division; A = the
    mean of |c1| + c2_A."""
    return K_COORD + 3 + 6 + 3 + nblk(P) + 2


def k_warp_cam(P, per_pixel=1):
    """a pixel's term (1: formed in float64, rounded once) + 6 shuffle levels + 3 wave adds + nblk ordered partials."""
    return per_pixel + 6 + 3 + nblk(P)


# ============================================================================================ f3
def single(depth, normal, mask, min_sdf, gt_depth, gt_normal, gt_mask, threshold, g4=(1.0, 1.0, 1.0, 1.0)):
    """All of f3. Arrays of any shape (P pixels; normals (..., 3)); gt_depth / gt_normal may be None. g4: the upstream gradients of the
    four means. Returns a dict: losses (4), loss_A (4), counts (4, int), member (4, P) bool, value (4, P), g_depth / g_normal / g_min_sdf
    and A_depth / A_normal / A_min_sdf (per entry)."""
    w = lambda a: None if a is None else np.asarray(a, dtype=np.float32).astype(np.float64)
    m, g = np.asarray(mask).reshape(-1) != 0, np.asarray(gt_mask).reshape(-1) != 0
    P = m.size
    q, t = w(min_sdf).reshape(-1), float(np.float32(threshold))
    g4 = [float(np.float32(v)) for v in g4]
    member, value, mag = np.zeros((4, P), dtype=bool), np.zeros((4, P)), np.zeros((4, P))
    member[0] = g & ~m                                                  # loss_utils.py:75   mask_gt = gt \ out
    member[1] = m & ~g                                                  # loss_utils.py:89   mask_out = out \ gt
    with np.errstate(invalid='ignore'):
        value[0] = np.where(member[0], np.maximum(q - t, 0.0), 0.0)     # loss_utils.py:81   max(min_sdf - threshold, 0)
        value[1] = np.where(member[1], np.maximum(t - q, 0.0), 0.0)     # loss_utils.py:94   max(threshold - min_sdf, 0)
    mag[0], mag[1] = np.abs(value[0]), np.abs(value[1])
    g_q, g_d, g_n = np.zeros(P), np.zeros(P), np.zeros((P, 3))
    A_q, A_d, A_n = np.zeros(P), np.zeros(P), np.zeros((P, 3))
    if gt_depth is not None:
        d, gd = w(depth).reshape(-1), w(gt_depth).reshape(-1)
        with np.errstate(invalid='ignore'):
            member[2] = m & g & (gd > 0.0) & (gd < 1e5)                 # loss_utils.py:118-121   gt_depth > 0 && < 1e5 (NaN: no)
        dd = np.where(member[2], d - np.where(member[2], gd, 0.0), 0.0)
        value[2] = mag[2] = np.abs(dd)                                  # loss_utils.py:127   |depth - gt_depth|
    if gt_normal is not None:
        n32 = np.asarray(normal, dtype=np.float32).reshape(-1, 3)
        with np.errstate(over='ignore', invalid='ignore', under='ignore'):
            nn32 = np.sqrt(n32[:, 0] * n32[:, 0] + n32[:, 1] * n32[:, 1] + n32[:, 2] * n32[:, 2])      # the float32 norm, as the kernel forms it
            member[3] = m & g & (nn32 != 0)                             # loss_utils.py:155-160   |n| != 0 in float32 (NaN != 0 holds)
        sel = member[3]
        n, b = n32[sel].astype(np.float64), w(gt_normal).reshape(-1, 3)[sel]
        nn, bn = np.sqrt((n * n).sum(1)), np.sqrt((b * b).sum(1))
        e = nn + EPS
        bh = b / (bn + EPS)[:, None]                                    # a zero gt normal: bh = 0, value 0, gradient 0
        parts = (n / e[:, None]) * bh
        value[3, sel], mag[3, sel] = -parts.sum(1), np.abs(parts).sum(1)         # loss_utils.py:165-169   -(n^ . b^)
    counts = member.sum(1)
    losses, loss_A = np.zeros(4), np.zeros(4)
    for k in range(4):                                                  # loss_utils.py:82-84 and the like: the mean over an empty set is 0
        if counts[k]:
            losses[k], loss_A[k] = value[k][member[k]].sum() / counts[k], mag[k][member[k]].sum() / counts[k]
    # gradients. The hinge's sub-gradient at an exact tie min_sdf == threshold is 0: the kernel tests (q - t) > 0, and q - t == 0 in
    # float32 exactly where q == t. (loss_oracle clamps; the reference's torch.max(x, zeros), loss_utils.py:81, 94, depends on the
    # torch version at a tie.) This is the kernel's rule, pinned.
    with np.errstate(invalid='ignore'):
        s0, s1 = member[0] & (q > t), member[1] & (q < t)
    if counts[0]:
        g_q[s0] += g4[0] / counts[0]
    if counts[1]:
        g_q[s1] -= g4[1] / counts[1]
    A_q = np.abs(g_q)
    if counts[2]:
        g_d = np.sign(dd) * (g4[2] / counts[2])                         # sign(0) = 0: depth == gt_depth has no gradient
        A_d = np.abs(g_d)
    if counts[3]:
        wgt = g4[3] / counts[3]
        nb = (n * bh).sum(1)
        t1, t2 = bh / e[:, None], nb[:, None] * n / (nn * e * e)[:, None]
        g_n[sel] = -wgt * (t1 - t2)
        A_n[sel] = abs(wgt) * (np.abs(t1) + np.abs(n * bh).sum(1)[:, None] * np.abs(n) / (nn * e * e)[:, None])
    return dict(losses=losses, loss_A=loss_A, counts=counts, member=member, value=value, g_depth=g_d, g_normal=g_n, g_min_sdf=g_q,
                A_depth=A_d, A_normal=A_n, A_min_sdf=A_q)


# ============================================================================================ f2
def _dot3(M, row, v, T=False):
    return (M[0][row] * v[0] + M[1][row] * v[1] + M[2][row] * v[2]) if T else (M[row][0] * v[0] + M[row][1] * v[1] + M[row][2] * v[2])


def warp(H, W, K, K_inv, thres_depth, z1, m1, z2, img1, img2, R1, T1, R2, T2, g_loss=1.0, dtype=np.float64):
    """All of f2 for the float32 inputs of distr_warp_loss_forward / _backward (K, K_inv: the float32 matrices inside distr_warp_cfg).
    Returns a dict; per-pixel arrays are over the image (P), zero off the valid set:
      valid, keep (bool), loss, loss_A, n_kept, n_valid, c1, c2 (P, 3), g_z, A_z (P), cam (24) = [g_R1 9 | g_T1 3 | g_R2 9 | g_T2 3], cam_A (24),
      terms (P, 24): every pixel's own contribution to cam; ix, iy, err2;
      margins: m_thres = |err^2 - thres|, m_grid = distance of (ix, iy) to the nearest grid line, m_color (P, 3) = |c1 - c2|;
      bounds of the same: b_thres, b_grid, b_color (from the float32 roundings ahead of each decision, module docstring);
      flat (P, 3): the four zero-padded corners of the channel are equal (its gradient is exactly 0 whatever sign(c1 - c2) is);
      ambiguous (P) bool; outside (P) int: how many of the four footprint corners lie outside view 2 (valid pixels)."""
    dt = dtype
    c = lambda a: np.asarray(a, dtype=np.float32).astype(dt)
    K, Ki, R1, T1, R2, T2 = c(K).reshape(3, 3), c(K_inv).reshape(3, 3), c(R1).reshape(3, 3), c(T1).reshape(3), c(R2).reshape(3, 3), c(T2).reshape(3)
    P = H * W
    z1, z2, img1, img2 = c(z1).reshape(P), c(z2).reshape(P), c(img1).reshape(P, 3), c(img2).reshape(P, 3)
    thres = dt(np.float32(thres_depth))
    valid = np.asarray(m1).reshape(P) != 0
    idx = np.nonzero(valid)[0]
    out = dict(valid=valid, n_valid=int(idx.size), keep=np.zeros(P, dtype=bool), c1=np.zeros((P, 3), dt), c2=np.zeros((P, 3), dt), g_z=np.zeros(P, dt),
               A_z=np.zeros(P), cam=np.zeros(24, dt), cam_A=np.zeros(24), terms=np.zeros((P, 24), dt), n_kept=0, loss_A=0.0,
               ambiguous=np.zeros(P, dtype=bool), outside=np.zeros(P, dtype=int), flat=np.zeros((P, 3), dtype=bool), c2_A=np.zeros((P, 3)))
    if idx.size == 0:                                                   # renderer_warp.py:111-113: no valid pixel -> loss 0, no gradient
        out['loss'] = dt(0.0)
        return out
    x, y = (idx % W).astype(dt), (idx // W).astype(dt)
    z = z1[idx]
    with np.errstate(all='ignore'):
        h = [Ki[a][0] * x + Ki[a][1] * y + Ki[a][2] for a in range(3)]
        r = [_dot3(R1, i, h, T=True) for i in range(3)]
        rn = np.sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2])
        e = rn + dt(EPS)
        d = [r[i] / e for i in range(3)]
        c1 = [-(R1[0][j] * T1[0] + R1[1][j] * T1[1] + R1[2][j] * T1[2]) for j in range(3)]
        pt = [d[a] * z + c1[a] for a in range(3)]                       # renderer_warp.py:23-28
        q = [_dot3(R2, a, pt) + T2[a] for a in range(3)]
        pr = [_dot3(K, a, q) for a in range(3)]                         # renderer_warp.py:31
        u, v = pr[0] / pr[2], pr[1] / pr[2]
        # loss_utils.py:17-24: normalise, and grid_sample(align_corners=True) un-normalises; for W = 1 the round trip gives ix = 0
        gx, gy = dt(2.0) * u / dt(max(W - 1, 1)) - dt(1.0), dt(2.0) * v / dt(max(H - 1, 1)) - dt(1.0)
        ix, iy = ((gx + dt(1.0)) / dt(2.0)) * dt(W - 1), ((gy + dt(1.0)) / dt(2.0)) * dt(H - 1)
        dix, diy = (1.0 if W > 1 else 0.0), (1.0 if H > 1 else 0.0)      # d ix / d u, d iy / d v of that round trip
        ok = (ix > -2.0) & (ix < W + 1.0) & (iy > -2.0) & (iy < H + 1.0)  # false for NaN / inf: every corner is outside
        fx, fy = np.where(ok, np.floor(ix), 0.0).astype(dt), np.where(ok, np.floor(iy), 0.0).astype(dt)
        tx, ty = ix - fx, iy - fy
        x0, y0 = fx.astype(np.int64), fy.astype(np.int64)
        n = idx.size
        d2, d2_mag, d2_x, d2_y = np.zeros(n, dt), np.zeros(n), np.zeros(n, dt), np.zeros(n, dt)
        val = np.zeros((2, 2, n, 3), dt)
        inside = np.zeros((2, 2, n), dtype=bool)
        wx, wy = [dt(1.0) - tx, tx], [dt(1.0) - ty, ty]
        for dy in range(2):
            for dx in range(2):
                xx, yy = x0 + dx, y0 + dy
                inb = ok & (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)   # zero padding
                inside[dy, dx] = inb
                xs, ys = np.where(inb, xx, 0), np.where(inb, yy, 0)
                xf, yf = xs.astype(dt), ys.astype(dt)
                hx, hy, hz = (Ki[a][0] * xf + Ki[a][1] * yf + Ki[a][2] for a in range(3))
                calib = hz / (np.sqrt(hx * hx + hy * hy + hz * hz) + dt(EPS))      # renderer_warp.py:65-68: Zdepth2 * calib_map
                dz = np.where(inb, z2[ys * W + xs] * calib, 0.0).astype(dt)
                d2 = d2 + dz * (wx[dx] * wy[dy])
                d2_mag = d2_mag + np.abs(dz * (wx[dx] * wy[dy]))
                d2_x, d2_y = d2_x + dz * wy[dy] * (1 if dx else -1), d2_y + dz * wx[dx] * (1 if dy else -1)
                val[dy, dx] = np.where(inb[:, None], img2[ys * W + xs], 0.0)
        err = pr[2] - d2
        err2 = err * err
        keep = err2 < thres                                             # renderer_warp.py:70-71 (NaN: not kept)
        c2 = sum(val[dy, dx] * (wx[dx] * wy[dy])[:, None] for dy in range(2) for dx in range(2))
        a1 = img1[idx]
        diff = a1 - c2
        n_kept = int(keep.sum())
        # renderer_warp.py:85: mean over kept pixels x 3 channels; of an empty kept set NaN, as torch.mean of an empty tensor
        loss = np.where(keep[:, None], np.abs(diff), 0.0).sum(dtype=dt) / dt(3.0 * n_kept) if n_kept else dt(np.nan)
        scale = dt(np.float32(g_loss)) / dt(3.0 * n_kept) if n_kept else dt(0.0)
        gc = -np.sign(diff) * scale                                     # sign(0) = 0
        gc = np.where(keep[:, None], gc, 0.0).astype(dt)
        # d c2 / d (ix, iy), zero-padded corners
        cx = (val[0, 1] - val[0, 0]) * wy[0][:, None] + (val[1, 1] - val[1, 0]) * wy[1][:, None]
        cy = (val[1, 0] - val[0, 0]) * wx[0][:, None] + (val[1, 1] - val[0, 1]) * wx[1][:, None]
        cross = val[1, 1] - val[1, 0] - val[0, 1] + val[0, 0]
        gix, giy = (gc * cx).sum(1) * dt(dix), (gc * cy).sum(1) * dt(diy)
        gpr = [gix / pr[2], giy / pr[2], -(gix * u + giy * v) / pr[2]]
        gq = [K[0][b] * gpr[0] + K[1][b] * gpr[1] + K[2][b] * gpr[2] for b in range(3)]
        gpt = [_dot3(R2, b, gq, T=True) for b in range(3)]
        gz_parts = [gpt[a] * d[a] for a in range(3)]
        gd = [gpt[a] * z for a in range(3)]
        dot = gd[0] * r[0] + gd[1] * r[1] + gd[2] * r[2]
        gr = [gd[i] / e - np.where(rn > 0, dot * r[i] / (rn * e * e), 0.0) for i in range(3)]
        terms = np.zeros((n, 24), dt)
        for j in range(3):
            for i in range(3):
                terms[:, j * 3 + i] = h[j] * gr[i] - gpt[i] * T1[j]     # R1: through the normalised ray, and c1_i = -sum_j R1[j][i] T1[j]
                terms[:, 12 + j * 3 + i] = gq[j] * pt[i]                # R2
            terms[:, 9 + j] = -(R1[j][0] * gpt[0] + R1[j][1] * gpt[1] + R1[j][2] * gpt[2])   # T1
            terms[:, 21 + j] = gq[j]                                    # T2
        terms = np.where(keep[:, None], np.nan_to_num(terms), 0.0).astype(dt)
        g_z = np.where(keep, np.nan_to_num(gz_parts[0] + gz_parts[1] + gz_parts[2]), 0.0)
        A_z = np.where(keep, np.nan_to_num(np.abs(gz_parts[0]) + np.abs(gz_parts[1]) + np.abs(gz_parts[2])), 0.0)
        # ---- decisions: margins and the bounds of the float32 roundings ahead of them
        Mx, My = (np.abs(u) + (W - 1)) * dix, (np.abs(v) + (H - 1)) * diy
        b_ix, b_iy = K_COORD * U * Mx, K_COORD * U * My
        fr = lambda a: np.abs(a - np.round(a))
        m_grid = np.minimum(np.where(dix > 0, fr(ix), np.inf), np.where(diy > 0, fr(iy), np.inf))
        b_grid = np.maximum(b_ix, b_iy)
        pt_mag = [np.abs(d[a] * z) + abs(R1[0][a] * T1[0]) + abs(R1[1][a] * T1[1]) + abs(R1[2][a] * T1[2]) for a in range(3)]
        q_mag = [abs(R2[a][0]) * pt_mag[0] + abs(R2[a][1]) * pt_mag[1] + abs(R2[a][2]) * pt_mag[2] + abs(T2[a]) for a in range(3)]
        pr2_mag = abs(K[2][0]) * q_mag[0] + abs(K[2][1]) * q_mag[1] + abs(K[2][2]) * q_mag[2]
        b_err = U * (K_PR * pr2_mag + K_D2 * d2_mag + np.abs(err)) + np.abs(d2_x) * b_ix + np.abs(d2_y) * b_iy
        b_thres = 2.0 * np.abs(err) * b_err + b_err * b_err + U * err2
        m_thres = np.abs(err2 - thres)
        c2_mag = sum(np.abs(val[dy, dx]) * (wx[dx] * wy[dy])[:, None] for dy in range(2) for dx in range(2))
        b_color = U * (K_C2 * c2_mag + np.abs(a1)) + np.abs(cx) * b_ix[:, None] + np.abs(cy) * b_iy[:, None]
        m_color = np.abs(diff)
        flat = (val[0, 0] == val[0, 1]) & (val[0, 0] == val[1, 0]) & (val[0, 0] == val[1, 1])
        amb = ~(m_thres >= b_thres)                                     # NaN margins count as ambiguous
        amb |= keep & ((m_grid < b_grid) | ((~flat) & (m_color > 0) & (m_color < b_color)).any(1))
        c2_A = (c2_mag + np.abs(cx) * Mx[:, None] + np.abs(cy) * My[:, None]).astype(np.float64)     # what a rounding of c2 is relative to
    full = lambda a, shape=(), t=dt: _scatter(P, idx, a, shape, t)
    out.update(keep=full(keep, t=bool), n_kept=n_kept, loss=loss, loss_A=float(np.where(keep[:, None], np.abs(a1) + c2_A, 0.0).sum() / (3.0 * n_kept)) if n_kept else 0.0,
               c1=full(np.where(keep[:, None], a1, 0.0), (3,)), c2=full(np.where(keep[:, None], c2, 0.0), (3,)), g_z=full(g_z), A_z=full(A_z, t=np.float64),
               terms=full(terms, (24,)), cam=terms.sum(0, dtype=dt), cam_A=np.abs(terms.astype(np.float64)).sum(0),
               ix=full(ix), iy=full(iy), err2=full(err2), m_thres=full(m_thres, t=np.float64), b_thres=full(b_thres, t=np.float64),
               m_grid=full(m_grid, t=np.float64), b_grid=full(b_grid, t=np.float64), m_color=full(m_color, (3,), np.float64),
               b_color=full(b_color, (3,), np.float64), flat=full(flat, (3,), bool), ambiguous=full(amb, t=bool),
               outside=full(4 - inside.sum((0, 1)), t=int), c2_A=full(c2_A, (3,), np.float64))
    return out


def _scatter(P, idx, a, shape, t):
    o = np.zeros((P,) + tuple(shape), dtype=t)
    o[idx] = a
    return o


def ratio(err, bar):
    """Largest err / bar over the entries; an entry whose bar is zero has to be exact."""
    err, bar = np.asarray(err, dtype=np.float64), np.asarray(bar, dtype=np.float64)
    if err.size == 0:
        return 0.0
    with np.errstate(divide='ignore', invalid='ignore'):
        return float(np.max(np.where(bar > 0, err / bar, np.where(err > 0, np.inf, 0.0))))
