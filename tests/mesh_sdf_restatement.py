"""numpy restatement of the signed-distance kernels (csrc/distr_mesh.hpp: k_sdf_pairs / k_sdf_finish / k_sdf_queries) for
tests/test_mesh_sdf_host.py and tests/test_gpu_mesh_sdf.py, in the operation order the header spells out.

dtype=np.float32 restates the kernel: elementwise float32 operations only (numpy neither fuses nor reorders them; its division and
square root are correctly rounded like the build's), so the squared distance and the nearest face come out bit for bit; the solid
angles differ from the GPU's only by the two arctan2 implementations. The sums follow the kernel: float32 over a tile of SDF_TILE
faces in face order, float64 over the tiles of a chunk of SDF_CHUNK faces, float64 over the chunks.
dtype=np.float64 is the same formulas in float64 with plain float64 sums: the yardstick the float32 results are measured against. The
skip rule is the kernel's in both: the float32 cross product decides."""
import numpy as np

from mesh_restatement import rnd_bits

SDF_TILE = 256
SDF_CHUNK = 1024
INV_2PI = 0.15915494309189535
REGIONS = ('vertex a', 'vertex b', 'edge ab', 'vertex c', 'edge ac', 'edge bc', 'interior')
_U64 = np.uint64


def face_records(verts, faces, dtype=np.float32):
    """(a, ab, ac) of `dtype` (F, 3) each and counted (F,) bool: the records k_sdf_pairs stages, with its skip rule (decided by the
    float32 cross product whatever the dtype)."""
    v = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    ok = ((f >= 0) & (f < len(v))).all(1)
    fs = np.where(ok[:, None], f, 0)
    a, b, c = v[fs[:, 0]], v[fs[:, 1]], v[fs[:, 2]]
    with np.errstate(invalid='ignore', over='ignore'):
        ab, ac = b - a, c - a
        nx = ab[:, 1] * ac[:, 2] - ab[:, 2] * ac[:, 1]
        ny = ab[:, 2] * ac[:, 0] - ab[:, 0] * ac[:, 2]
        nz = ab[:, 0] * ac[:, 1] - ab[:, 1] * ac[:, 0]
    fin = np.isfinite(a).all(1) & np.isfinite(b).all(1) & np.isfinite(c).all(1)
    ok = ok & fin & ~((nx == 0) & (ny == 0) & (nz == 0))
    if dtype != np.float32:
        with np.errstate(invalid='ignore', over='ignore'):
            a, b, c = a.astype(dtype), b.astype(dtype), c.astype(dtype)
            ab, ac = b - a, c - a
    return a, ab, ac, ok


def _dot(u, v):
    return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]


def pair_terms(verts, faces, Q, dtype=np.float32):
    """Per (query, face): dist2 (nq, F), half solid angle (nq, F), region (nq, F) index into REGIONS. Skipped faces: +inf, 0, -1."""
    a, ab, ac, ok = face_records(verts, faces, dtype)
    Q = np.ascontiguousarray(Q, np.float32).reshape(-1, 3)
    T = dtype
    one, zero = T(1), T(0)
    q = [Q[:, k].astype(T)[:, None] for k in range(3)]
    a_ = [np.where(ok, a[:, k], 0).astype(T)[None, :] for k in range(3)]
    ab_ = [np.where(ok, ab[:, k], 0).astype(T)[None, :] for k in range(3)]
    ac_ = [np.where(ok, ac[:, k], 0).astype(T)[None, :] for k in range(3)]
    with np.errstate(invalid='ignore', divide='ignore', over='ignore', under='ignore'):
        ap = [q[k] - a_[k] for k in range(3)]
        bp = [ap[k] - ab_[k] for k in range(3)]
        cp = [ap[k] - ac_[k] for k in range(3)]
        d1, d2 = _dot(ab_, ap), _dot(ac_, ap)
        d3, d4 = _dot(ab_, bp), _dot(ac_, bp)
        d5, d6 = _dot(ab_, cp), _dot(ac_, cp)
        vc = d1 * d4 - d3 * d2
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        e43, e56 = d4 - d3, d5 - d6
        sn, tn = vb, vc
        sd = (va + vb) + vc
        td = sd
        reg = np.full(sd.shape, 6, np.int8)
        ones, zeros = np.full(sd.shape, one, T), np.full(sd.shape, zero, T)

        def put(cond, r, s_n, s_d, t_n, t_d):
            nonlocal sn, sd, tn, td, reg
            sn, sd, tn, td = np.where(cond, s_n, sn), np.where(cond, s_d, sd), np.where(cond, t_n, tn), np.where(cond, t_d, td)
            reg = np.where(cond, np.int8(r), reg)
        put((va <= 0) & (e43 >= 0) & (e56 >= 0), 5, ones, ones, e43, e43 + e56)
        put((vb <= 0) & (d2 >= 0) & (d6 <= 0), 4, zeros, ones, d2, d2 - d6)
        put((d6 >= 0) & (d5 <= d6), 3, zeros, ones, ones, ones)
        put((vc <= 0) & (d1 >= 0) & (d3 <= 0), 2, d1, d1 - d3, zeros, ones)
        put((d3 >= 0) & (d4 <= d3), 1, ones, ones, zeros, ones)
        put((d1 <= 0) & (d2 <= 0), 0, zeros, ones, zeros, ones)
        s, t = sn / sd, tn / td
        e = [np.where(reg == 5, ac_[k] - ab_[k], ac_[k]) for k in range(3)]      # edge bc: b + w (c - b) with b = a + ab
        d = [q[k] - ((a_[k] + s * ab_[k]) + t * e[k]) for k in range(3)]
        dist2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
        A = [a_[k] - q[k] for k in range(3)]
        B = [A[k] + ab_[k] for k in range(3)]
        Cc = [A[k] + ac_[k] for k in range(3)]
        cr = [B[1] * Cc[2] - B[2] * Cc[1], B[2] * Cc[0] - B[0] * Cc[2], B[0] * Cc[1] - B[1] * Cc[0]]
        num = _dot(A, cr)
        la, lb, lc = np.sqrt(_dot(A, A)), np.sqrt(_dot(B, B)), np.sqrt(_dot(Cc, Cc))
        den = ((((la * lb) * lc) + _dot(A, B) * lc) + _dot(B, Cc) * la) + _dot(Cc, A) * lb
        half = np.arctan2(num, den)
    assert dist2.dtype == T and half.dtype == T
    okb = np.broadcast_to(ok[None, :], dist2.shape)
    dist2 = np.where(okb & (dist2 < np.inf), dist2, T(np.inf))          # a NaN or an overflow never wins
    return dist2, np.where(okb, half, zero), np.where(okb, reg, np.int8(-1))


def _half_sums(half, dtype):
    """Sum over the faces of (nq, F) half solid angles, float64 (nq,): the kernel's order for float32, plain float64 otherwise."""
    if dtype == np.float64:
        return np.cumsum(half, axis=1)[:, -1]                          # in face order (np.sum would pair them up)
    nq, nf = half.shape
    ntiles = (nf + SDF_TILE - 1) // SDF_TILE
    pad = np.zeros((nq, ntiles * SDF_TILE), np.float32)
    pad[:, :nf] = half
    pad = pad.reshape(nq, ntiles, SDF_TILE)
    acc = np.zeros((nq, ntiles), np.float32)
    for k in range(SDF_TILE):                                          # face order inside a tile, float32
        acc = acc + pad[:, :, k]
    per = SDF_CHUNK // SDF_TILE
    tot = np.zeros(nq, np.float64)
    for c0 in range(0, ntiles, per):                                   # chunk order
        ch = np.zeros(nq, np.float64)
        for t in range(c0, min(c0 + per, ntiles)):                     # tile order inside a chunk
            ch = ch + acc[:, t].astype(np.float64)
        tot = tot + ch
    return tot


def signed_distance(verts, faces, Q, dtype=np.float32, max_elems=1 << 21):
    """(sdf, dist2, winding, face): float32 arrays and int32 for dtype float32 (k_sdf_finish's outputs), float64 arrays for float64.
    Row blocks of at most max_elems pairs: rows are independent."""
    Q = np.ascontiguousarray(Q, np.float32).reshape(-1, 3)
    nf = len(np.asarray(faces).reshape(-1, 3))
    nq = len(Q)
    T = dtype
    sdf, d2o, w, face = np.empty(nq, T), np.empty(nq, T), np.empty(nq, T), np.empty(nq, np.int32)
    rows = max(1, max_elems // max(1, nf))
    for i0 in range(0, nq, rows):
        dist2, half, _ = pair_terms(verts, faces, Q[i0:i0 + rows], T)
        best = dist2.min(1)
        fi = dist2.argmin(1).astype(np.int32)                          # the first of equal minima: the lowest face index
        fi[~(best < np.inf)] = -1
        ww = (_half_sums(half, T) * INV_2PI).astype(T)
        with np.errstate(invalid='ignore'):
            out = np.where(np.abs(ww) > T(0.5), T(-1), T(1)) * np.sqrt(best)
        bad = ~np.isfinite(Q[i0:i0 + rows]).all(1)
        out[bad], best[bad], ww[bad], fi[bad] = np.nan, np.nan, np.nan, -1
        sdf[i0:i0 + rows], d2o[i0:i0 + rows], w[i0:i0 + rows], face[i0:i0 + rows] = out, best, ww, fi
    return sdf, d2o, w, face


# ------------------------------------------------------------------------------------------------------------ query points
def _word(seed, n):
    """W(n) = rnd_bits(seed, n, 3) split into its two 24-bit numbers (hi, lo) as uint64 arrays."""
    w = rnd_bits(seed, n, 3)
    return w >> _U64(40), (w >> _U64(8)) & _U64(0xffffff)


def normals(seed, ns, dtype=np.float32):
    """(ns, 6) standard normals of the surface points 0 .. ns - 1 (Box-Muller on the words 8 i, 8 i + 1, 8 i + 2)."""
    T = dtype
    i = np.arange(ns, dtype=np.uint64)
    z = np.empty((ns, 6), T)
    two_pi = np.float32(6.2831855) if T == np.float32 else np.float64(2 * np.pi)
    for m in range(3):
        hi, lo = _word(seed, i * _U64(8) + _U64(m))
        u1 = (hi + _U64(1)).astype(T) * T(2.0 ** -24)
        u2 = lo.astype(T) * T(2.0 ** -24)
        r = np.sqrt(T(-2) * np.log(u1))
        ang = two_pi * u2
        z[:, 2 * m], z[:, 2 * m + 1] = r * np.cos(ang), r * np.sin(ang)
    assert z.dtype == T
    return z


def uniforms(seed, nu):
    """(nu, 3) float32 in [0, 1): the 24-bit numbers of the words 8 j + 4 (hi, lo) and 8 j + 5 (hi), times 2^-24 (exact)."""
    j = np.arange(nu, dtype=np.uint64)
    h0, l0 = _word(seed, j * _U64(8) + _U64(4))
    h1, _ = _word(seed, j * _U64(8) + _U64(5))
    return np.stack([h0, l0, h1], 1).astype(np.float32) * np.float32(2.0 ** -24)


def sdf_queries(surf, sigma_a, sigma_b, n_uniform, half_extent, seed, dtype=np.float32):
    """k_sdf_queries restated: (2 ns + n_uniform, 3) of `dtype`; sigma and half_extent are the float32 numbers the kernel gets."""
    T = dtype
    p = np.ascontiguousarray(surf, np.float32).reshape(-1, 3).astype(T)
    ns = len(p)
    z = normals(seed, ns, T)
    sa, sb, h = T(np.float32(sigma_a)), T(np.float32(sigma_b)), T(np.float32(half_extent))
    out = np.empty((2 * ns + n_uniform, 3), T)
    out[0:2 * ns:2] = p + sa * z[:, :3]
    out[1:2 * ns:2] = p + sb * z[:, 3:]
    out[2 * ns:] = (T(2) * uniforms(seed, n_uniform).astype(T) - T(1)) * h
    return out


# ------------------------------------------------------------------------------------------------------------ test meshes
def box(half=0.5, inward=False):
    """The 12-triangle cube [-half, half]^3, normals outwards (or inwards): (verts (8, 3) float32, faces (12, 3) int32)."""
    v = np.array([[x, y, z] for x in (-half, half) for y in (-half, half) for z in (-half, half)], np.float32)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]      # counter-clockwise from outside
    f = np.array([t for q in quads for t in ((q[0], q[1], q[2]), (q[0], q[2], q[3]))], np.int32)
    return v, (f[:, ::-1].copy() if inward else f)


def box_sdf(Q, half=0.5):
    """Closed-form signed distance to the cube's surface, float64."""
    d = np.abs(np.asarray(Q, np.float64)) - half
    return np.linalg.norm(np.maximum(d, 0), axis=1) + np.minimum(d.max(1), 0)


# one triangle with dyadic corners in the plane z = 1: a = (0, 0), b = (4, 0), c = (0, 4); every number below is exact in float32
TRI_V = np.array([[0, 0, 1], [4, 0, 1], [0, 4, 1]], np.float32)
TRI_F = np.array([[0, 1, 2]], np.int32)
# query, region, closest point
TRI_CASES = [
    ((-1.0, -2.0, 1.5), 'vertex a', (0, 0, 1)),
    ((6.0, -1.0, 0.5), 'vertex b', (4, 0, 1)),
    ((1.5, -2.0, 1.0), 'edge ab', (1.5, 0, 1)),
    ((-1.0, 6.0, 2.0), 'vertex c', (0, 4, 1)),
    ((-3.0, 2.5, 1.25), 'edge ac', (0, 2.5, 1)),
    ((4.0, 3.0, 1.0), 'edge bc', (2.5, 1.5, 1)),
    ((1.0, 1.5, -2.0), 'interior', (1, 1.5, 1)),
    # on a vertex, on each edge and inside the face, in its plane: distance exactly 0
    ((4.0, 0.0, 1.0), 'vertex b', (4, 0, 1)),
    ((0.0, 0.0, 1.0), 'vertex a', (0, 0, 1)),
    ((0.0, 4.0, 1.0), 'vertex c', (0, 4, 1)),
    ((2.5, 0.0, 1.0), 'edge ab', (2.5, 0, 1)),
    ((0.0, 0.75, 1.0), 'edge ac', (0, 0.75, 1)),
    ((1.0, 3.0, 1.0), 'edge bc', (1, 3, 1)),
    ((1.25, 0.5, 1.0), 'interior', (1.25, 0.5, 1)),
]
