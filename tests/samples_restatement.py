"""A plain restatement of the list stages around the decoder: the depth-sample kernels (csrc/distr_samples.hpp), the colour stage's
point list and camera sums without lights (csrc/distr_color_batch.hpp). CPU only; float64 unless the caller hands in another type.

Every constant enters as the float32 value the library receives (K_inv, M, R, T, depth, normal, draws) and is widened by the caller;
nothing here rounds. `points` and `surface_points` are written with plain arithmetic on their arguments, so the same text runs on
float64 numpy arrays (the reference), float32 numpy arrays (what a correct f32 implementation gives, tests/test_samples_edges_host.py)
and float64 torch tensors under autograd (the check of `camera_terms`).

Layouts are those of include/distr_samples.h: view v owns m N_v consecutive list entries, [k][i] inside a view (k = 0 p + o / 1 p - o,
or the draw; i = the view's valid pixel in row-major order).

The bar of the camera sums, `rounding_bar`, is k 2^-24 A: A = the float64 sum of the absolute per-pixel contributions to an entry
(carried through g_R = ray - T (x) g_c, g_T = -R g_c), k = `rounding_count`, the number of float32 roundings on the longest path from
a pixel's inputs to the output, counted from the kernels with every float32 multiplication, addition, division and square root rounding
once (the library is built without contraction, and a fused multiply-add would only remove roundings):

    depth samples (k_samp_cam_bwd, k_samp_cam_fin)                  colour stage (k_cb_cam_bwd, k_cb_cam_fin)
      the pixel's twelve terms: formed in float64 from the          h = K_inv (x, y, 1)   mul, add, add          3
      float32 inputs (make_ray64, z, g_q, g_d, g_r, h_j g_r),       r = R^T h             mul, add, add          6
      rounded to float32 ONCE                              1         rn = |r|              mul, add, add, sqrt   10
                                                                    e = rn + 1e-12        add                   11
                                                                    g_q = M g_p           mul, add, add          3
                                                                    g_d = g_q z           mul                    4
                                                                    dot = g_d . r         mul, add, add          9
                                                                    dot r_i / (rn e e)    mul | mul, mul (13) | div   14
                                                                    g_r = g_d / e - that  sub                   15
                                                                    h_j g_r               mul                   16
      acc += term        MPER serial adds                  + 8                                                 + 8
      LDS tree of the block          8 levels              + 8                                                 + 8
      cam_fin: thread-serial run     ceil(nb / 256) adds   + ceil(nb / 256)
      cam_fin: LDS tree              8 levels              + 8                                                 + 8
      g_T = -(R0 c0 + R1 c1 + R2 c2) mul, add, add         + 3   (g_R: mul, sub)                               + 3

    k = 28 + ceil(nb / 256) for the depth samples, whatever the mode and `number` (29; the 257-block case: 30), and 43 + ceil(nb / 256) for
    the colour stage (44; 257 blocks: 45). The float64 operations inside a pixel's terms err by 2^-53 each and are not counted.

Why the depth samples form a pixel's terms in float64. A takes the absolute value of a pixel's finished contribution. Inside it,
g_r = g_d / e - (g_d . r) r / (rn e^2) is a difference (the part of g_d along the ray is removed, component by component), and g_d is a
sum over the pixel's list entries; where they cancel, the roundings of the parts are not small against the result. Over hundreds of
pixels that is invisible; a sum that holds ONE pixel is that one difference, and a float32 evaluation of the closed form (what
k_samp_cam_bwd did before; `camera_terms(dtype=np.float32)`) is off by more than the 47 + m roundings it has, times A, on 5 to 12 per cent of single
pixels, up to 118 times (tests/test_samples_edges_host.py prints the figures). The colour stage's kernel still works in float32: its
sums are asserted with A like the others, and `B` -- A with the absolute value taken of every product inside the pixel's arithmetic
too, which bounds a single pixel's float32 roundings -- is printed next to it and asserted only for the one-hot runs of the colour
stage, which the tests add on their own account.
"""
import numpy as np

MB, MPER = 256, 8
MTILE = MB * MPER
SURFACE, FREESPACE = 'surface', 'freespace'


def valid(depth):
    """depth (V, ...) float32 -> ([row-major indices of the valid pixels of view v], [N_v]): 0 < d < 1e5, compared in float64."""
    d = np.asarray(depth, dtype=np.float32)
    d = d.reshape(d.shape[0], -1).astype(np.float64)
    index = [np.nonzero((row > 0.0) & (row < 1e5))[0] for row in d]
    return index, [int(i.size) for i in index]


def _ray(Ki, R, x, y):
    h = [Ki[a][0] * x + Ki[a][1] * y + Ki[a][2] for a in range(3)]
    hn = (h[0] * h[0] + h[1] * h[1] + h[2] * h[2]) ** 0.5
    calib = h[2] / (hn + 1e-12)
    r = [R[0][i] * h[0] + R[1][i] * h[1] + R[2][i] * h[2] for i in range(3)]
    rn = (r[0] * r[0] + r[1] * r[1] + r[2] * r[2]) ** 0.5
    e = rn + 1e-12
    return h, calib, r, rn, e, [r[i] / e for i in range(3)]


def _point(M, R, T, d, z):
    c = [-(R[0][i] * T[0] + R[1][i] * T[1] + R[2][i] * T[2]) for i in range(3)]
    q = [d[i] * z + c[i] for i in range(3)]
    return [M[0][i] * q[0] + M[1][i] * q[1] + M[2][i] * q[2] for i in range(3)]


def _xy(index, W, like, xp):
    index = np.asarray(index)
    return xp.asarray(index % W, dtype=like.dtype), xp.asarray(index // W, dtype=like.dtype)


def points(mode, K_inv, M, RT, depth, index, W, normal=None, draws=None, xp=np):
    """The point list of ONE view: (m N, 3) in the type of `depth`. RT (3, 4); depth (P,); index: the view's valid pixels; SURFACE:
    normal (P, 3), draws = eta (N,); FREESPACE: draws = ratio (number, N)."""
    x, y = _xy(index, W, depth, xp)
    R = [[RT[j][i] for i in range(3)] for j in range(3)]
    T = [RT[j][3] for j in range(3)]
    _, calib, _, _, _, d = _ray(K_inv, R, x, y)
    z = depth[index] / calib
    if mode == SURFACE:
        p = _point(M, R, T, d, z)
        n = normal[index]
        o = [(M[0][i] * n[:, 0] + M[1][i] * n[:, 1] + M[2][i] * n[:, 2]) * draws for i in range(3)]
        return xp.concatenate([xp.stack([p[i] + o[i] for i in range(3)], -1), xp.stack([p[i] - o[i] for i in range(3)], -1)], 0)
    return xp.concatenate([xp.stack(_point(M, R, T, d, z * draws[k]), -1) for k in range(draws.shape[0])], 0)


def surface_points(K_inv, M, R, T, zdepth, index, W, xp=np):
    """The colour stage's points of ONE view: the same formula with zdepth (P,) given directly; R (3, 3), T (3,) -> (N, 3)."""
    x, y = _xy(index, W, zdepth, xp)
    d = _ray(K_inv, R, x, y)[5]
    return xp.stack(_point(M, R, T, d, zdepth[index]), -1)


def _camera_core(K_inv, M, R, T, x, y, zs, gps):
    """zs: m arrays (N,), the depth along the ray of list entry k; gps: m arrays (N, 3), its upstream gradient."""
    h, _, r, rn, e, _ = _ray(K_inv, R, x, y)
    gd, gc = [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]
    for z, gp in zip(zs, gps):
        for j in range(3):
            gq = M[j][0] * gp[:, 0] + M[j][1] * gp[:, 1] + M[j][2] * gp[:, 2]
            gd[j] = gd[j] + gq * z
            gc[j] = gc[j] + gq
    dot = gd[0] * r[0] + gd[1] * r[1] + gd[2] * r[2]
    gr = [gd[i] / e - dot * r[i] / (rn * e * e) for i in range(3)]
    terms = np.stack([h[j] * gr[i] for j in range(3) for i in range(3)] + [gc[i] + 0.0 * x for i in range(3)], -1)     # (N, 12)
    s, a = terms.sum(0), np.abs(terms).sum(0)
    # the same closed form with every product and quotient replaced by its absolute value: what bounds the roundings of one pixel's
    # own arithmetic when its differences cancel (a sum that holds a single pixel)
    ga, ca = [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]
    for z, gp in zip(zs, gps):
        for j in range(3):
            gq = abs(M[j][0] * gp[:, 0]) + abs(M[j][1] * gp[:, 1]) + abs(M[j][2] * gp[:, 2])
            ga[j] = ga[j] + gq * abs(z)
            ca[j] = ca[j] + gq
    dota = ga[0] * abs(r[0]) + ga[1] * abs(r[1]) + ga[2] * abs(r[2])
    gra = [ga[i] / e + dota * abs(r[i]) / (rn * e * e) for i in range(3)]
    parts = np.stack([abs(h[j]) * gra[i] for j in range(3) for i in range(3)] + [ca[i] + 0.0 * x for i in range(3)], -1).sum(0)
    R, T = np.asarray(R, dtype=np.float64), np.asarray(T, dtype=np.float64)
    g_RT, A_RT, B_RT = compose(s, R, T), compose(a, np.abs(R), np.abs(T), sign=1.0), compose(parts, np.abs(R), np.abs(T), sign=1.0)
    return dict(terms=terms, sum=s, abs=a, R=R, T=T, g_R=g_RT[:, :3], g_T=g_RT[:, 3], A_R=A_RT[:, :3], A_T=A_RT[:, 3], g_RT=g_RT, A_RT=A_RT,
                B_RT=B_RT)


def compose(t12, R, T, sign=-1.0):
    """Twelve sums -> (3, 4) = [ray - T (x) g_c | -R g_c]; sign = 1 with |R|, |T| carries sums of absolute values through."""
    t12 = np.asarray(t12, dtype=np.float64)
    return np.concatenate([t12[:9].reshape(3, 3) + sign * np.outer(T, t12[9:]), (sign * (R @ t12[9:]))[:, None]], 1)


def pixel_share(ct, i, bar):
    """Largest |contribution of list pixel i to an entry of g_RT| / that entry's bar: above 1, the sum fails without the pixel."""
    with np.errstate(divide='ignore', invalid='ignore'):
        return float(np.nanmax(np.abs(compose(ct['terms'][i], ct['R'], ct['T'])) / bar))


def camera_terms(mode, K_inv, M, RT, depth, index, W, g_xyz, draws=None, dtype=np.float64):
    """ONE view of the depth samples, float64 numpy. g_xyz (m N, 3): the gradient at the view's list entries. Per valid pixel the twelve
    contributions in closed form (ray_backward_acc and the M pull-back): nine of the ray part, h_j (g_d_i / e - (g_d . r) r_i / (rn e^2)),
    and three of g_c. Returns their sums ('sum'), sums of absolute values ('abs'), the per-pixel 'terms' (N, 12), g_RT (3, 4) =
    [ray - T (x) g_c | -R g_c] and A_RT, the absolute sums carried through the same composition; B_RT: the same with the absolute value
    taken of every product inside a pixel's own arithmetic as well (B >= A; module docstring). dtype float32 (with float32 inputs):
    the per-pixel terms and their sums in float32, as a plain f32 implementation has them (the composition stays float64)."""
    RT = np.asarray(RT, dtype=dtype)
    x, y = _xy(index, W, depth, np)
    R, T = RT[:, :3], RT[:, 3]
    N = len(index)
    z = depth[index] / _ray(K_inv, R, x, y)[1]
    m = 2 if mode == SURFACE else draws.shape[0]
    zs = [z if mode == SURFACE else z * draws[k] for k in range(m)]
    return _camera_core(K_inv, M, R, T, x, y, zs, [g_xyz[k * N:(k + 1) * N] for k in range(m)])


def camera_terms_color(K_inv, M, R, T, zdepth, index, W, g_xyz):
    """ONE view of the colour stage without lights: g_xyz (N, 3); as camera_terms, with g_R (3, 3), g_T (3,) apart."""
    x, y = _xy(index, W, zdepth, np)
    return _camera_core(K_inv, M, np.asarray(R, dtype=np.float64), np.asarray(T, dtype=np.float64), x, y, [zdepth[index]], [g_xyz])


def rounding_count(stage, n_valid):
    """k of the module docstring. stage 'samples' or 'color'."""
    nb = max(1, -(-int(n_valid) // MTILE))
    return (28 if stage == 'samples' else 43) + -(-nb // MB)


def rounding_bar(A, stage, n_valid):
    """k 2^-24 A, entry by entry (A_RT of camera_terms; B_RT for the bar that covers a single pixel in float32)."""
    return rounding_count(stage, n_valid) * 2.0 ** -24 * np.asarray(A, dtype=np.float64)


def points_bar(ref):
    """4 2^-23 max(1, max |p|): the 'few ulp of the largest coordinate' of test_equals_composed_helpers."""
    ref = np.asarray(ref)
    return 4 * 2.0 ** -23 * max(1.0, float(np.abs(ref).max()) if ref.size else 0.0)
