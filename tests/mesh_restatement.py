"""numpy float32 restatement of the GPU marching cubes (csrc/distr_mesh.hpp: k_mc_classify / k_mc_compact / k_mc_faces), read from
the same table, for tests/test_gpu_mesh.py. Vertices: one per sign-changing grid edge, ordered by (owning grid point, axis x < y < z),
t = a0 / (a0 - a1) with a = value - level and coord = origin + voxel_size * (index + t), in float32 without fused multiply-adds; faces
ordered by (cell = its lowest corner, table order).

Further down, for the same tests: the counter-based random bits (mix64 / rnd_bits), the area-weighted surface sampling (k_area_scan +
k_sample: float64 areas, np.cumsum, searchsorted, folded parallelogram in float32) and the brute-force nearest squared distance
(k_nearest: elementwise float32, minimum over B). tests/test_mesh_host.py checks these restatements on the CPU."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MESH_HPP = os.path.join(ROOT, 'dist-renderer_amd', 'csrc', 'distr_mesh.hpp')
CORNERS = [(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1)]


def _c_array(name, shape):
    src = open(MESH_HPP).read()
    m = re.search(r'%s\[[^\]]*\]\[[^\]]*\]\s*=\s*\{(.*?)\};' % name, src, re.S)
    vals = [int(v) for v in re.findall(r'-?\d+', m.group(1))]
    return np.array(vals, dtype=np.int64).reshape(shape)


def tables():
    """(kMcTri (256, 16), kMcEdge (12, 4)) as committed in the C++ source."""
    return _c_array('kMcTri', (256, 16)), _c_array('kMcEdge', (12, 4))


def marching_cubes(grid, level=0.0, origin=(-1.0, -1.0, -1.0), voxel_size=None):
    tri, edge = tables()
    g = np.ascontiguousarray(grid, dtype=np.float32)
    nx, ny, nz = g.shape
    if voxel_size is None:
        voxel_size = [2.0 / (n - 1) for n in g.shape]
    vs = np.broadcast_to(np.asarray(voxel_size, np.float32), (3,))
    org = np.broadcast_to(np.asarray(origin, np.float32), (3,))
    lev = np.float32(level)
    ins = g < lev
    em = np.zeros(g.shape, np.int64)
    em[:-1] |= (ins[:-1] != ins[1:]).astype(np.int64)
    em[:, :-1] |= (ins[:, :-1] != ins[:, 1:]).astype(np.int64) << 1
    em[:, :, :-1] |= (ins[:, :, :-1] != ins[:, :, 1:]).astype(np.int64) << 2
    emf = em.reshape(-1)
    nv = (emf & 1) + ((emf >> 1) & 1) + ((emf >> 2) & 1)
    vbase = np.concatenate([[0], np.cumsum(nv)[:-1]])
    # vertices
    flat = g.reshape(-1)
    step = np.array([ny * nz, nz, 1])
    keys = np.concatenate([np.nonzero((emf >> ax) & 1)[0] * 3 + ax for ax in range(3)])
    keys.sort()
    p, ax = keys // 3, keys % 3
    ijk = np.stack(np.unravel_index(p, g.shape), 1).astype(np.float32)
    with np.errstate(invalid='ignore', divide='ignore'):       # NaN / inf grid values: the kernel's IEEE results, no warning
        a0 = flat[p] - lev
        a1 = flat[p + step[ax]] - lev
        t = a0 / (a0 - a1)
    verts = np.empty((len(p), 3), np.float32)
    for d in range(3):
        td = np.where(ax == d, t, np.float32(0))
        verts[:, d] = org[d] + vs[d] * (ijk[:, d] + td)
    # faces
    code = np.zeros((nx - 1, ny - 1, nz - 1), np.int64)
    for q, (cx, cy, cz) in enumerate(CORNERS):
        code |= ins[cx:nx - 1 + cx, cy:ny - 1 + cy, cz:nz - 1 + cz].astype(np.int64) << q
    ci, cj, ck = np.nonzero((code != 0) & (code != 255))
    cc = code[ci, cj, ck]
    cp = (ci * ny + cj) * nz + ck
    order = np.argsort(cp, kind='stable')
    cc, cp = cc[order], cp[order]
    rows = tri[cc]                                   # (M, 16)
    e = rows[:, :15].reshape(-1, 5, 3)
    valid = e[:, :, 0] >= 0
    es = np.where(e >= 0, e, 0)
    q = cp[:, None, None] + edge[es, 0] * ny * nz + edge[es, 1] * nz + edge[es, 2]
    axis = edge[es, 3]
    emq = emf[q]
    below = emq & ((1 << axis) - 1)
    idx = vbase[q] + (below & 1) + ((below >> 1) & 1)
    faces = idx[valid].astype(np.int32).reshape(-1, 3)
    return verts, faces


def active_points(grid, level=0.0):
    """How many grid points k_mc_compact lists as active: those that own a sign-changing edge or whose cell has triangles (a cube
    index other than 0 and 255). k_mc_faces runs one thread per active point."""
    g = np.ascontiguousarray(grid, dtype=np.float32)
    nx, ny, nz = g.shape
    ins = g < np.float32(level)
    act = np.zeros(g.shape, bool)
    act[:-1] |= ins[:-1] != ins[1:]
    act[:, :-1] |= ins[:, :-1] != ins[:, 1:]
    act[:, :, :-1] |= ins[:, :, :-1] != ins[:, :, 1:]
    n_in = np.zeros((nx - 1, ny - 1, nz - 1), np.int64)
    for cx, cy, cz in CORNERS:
        n_in += ins[cx:nx - 1 + cx, cy:ny - 1 + cy, cz:nz - 1 + cz]
    act[:-1, :-1, :-1] |= (n_in != 0) & (n_in != 8)
    return int(act.sum())


def sphere_grid(N, center, r, shape=None):
    shape = shape or (N, N, N)
    axes = [np.linspace(-1, 1, n).astype(np.float32) for n in shape]
    X, Y, Z = np.meshgrid(*axes, indexing='ij')
    return (np.sqrt((X - center[0]) ** 2 + (Y - center[1]) ** 2 + (Z - center[2]) ** 2) - r).astype(np.float32)


def torus_grid(N, center, R, r):
    ax = np.linspace(-1, 1, N).astype(np.float32)
    X, Y, Z = np.meshgrid(ax, ax, ax, indexing='ij')
    X, Y, Z = X - center[0], Y - center[1], Z - center[2]
    q = np.sqrt(X ** 2 + Y ** 2) - R
    return (np.sqrt(q ** 2 + Z ** 2) - r).astype(np.float32)


def edge_use_counts(faces):
    e = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]])
    e = np.sort(e, 1)
    _, counts = np.unique(e, axis=0, return_counts=True)
    return counts


def euler(verts, faces):
    return len(np.unique(faces)) - len(edge_use_counts(faces)) + len(faces)


def signed_volume_area(verts, faces):
    v = verts.astype(np.float64)
    a, b, c = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    vol = np.einsum('ij,ij->i', a, np.cross(b, c)).sum() / 6.0
    area = 0.5 * np.linalg.norm(np.cross(b - a, c - a), axis=1).sum()
    return vol, area


def directed_edge_counts(faces):
    """Per undirected edge (lo, hi): how many faces run it lo -> hi and how many hi -> lo. A consistently oriented closed surface has
    the two equal on every edge (both 1 on a 2-manifold)."""
    f = np.asarray(faces, np.int64)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    fwd = e[:, 0] < e[:, 1]
    key = e.min(1) * (int(f.max()) + 1 if len(f) else 1) + e.max(1)
    uniq, inv = np.unique(key, return_inverse=True)
    inv = inv.reshape(-1)
    return np.bincount(inv[fwd], minlength=len(uniq)), np.bincount(inv[~fwd], minlength=len(uniq))


# ------------------------------------------------------------------------------------------------------------ surface sampling
_U64 = np.uint64


def mix64(z):
    """splitmix64 finaliser of csrc/distr_mesh.hpp on uint64 arrays (wrapping arithmetic)."""
    z = np.atleast_1d(np.asarray(z, dtype=np.uint64)).copy()
    with np.errstate(over='ignore'):
        z += _U64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> _U64(30))) * _U64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> _U64(27))) * _U64(0x94D049BB133111EB)
    return z ^ (z >> _U64(31))


def rnd_bits(seed, i, k):
    """Counter-based random bits of (seed, sample i, k): mix64(mix64(seed) ^ mix64(4 * i + k)), uint64 array of i's shape."""
    i = np.atleast_1d(np.asarray(i, dtype=np.uint64))
    with np.errstate(over='ignore'):
        c = i * _U64(4) + _U64(k)
    return mix64(mix64(_U64(int(seed) & (2 ** 64 - 1))) ^ mix64(c))


def face_areas(verts, faces):
    """float64 areas as face_area computes them; a face naming a vertex outside [0, nv) has area 0."""
    v = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    ok = ((f >= 0) & (f < len(v))).all(1)
    fs = np.where(ok[:, None], f, 0)
    a, b, c = (v[fs[:, k]].astype(np.float64) for k in range(3))
    e1, e2 = b - a, c - a
    cx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
    cy = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
    cz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    area = 0.5 * np.sqrt(cx * cx + cy * cy + cz * cz)
    area[~ok] = 0.0
    return area, ok


def sample_surface(verts, faces, n, seed):
    """k_sample restated: (points float32 (n, 3), face index int64 (n,), band float64 (n,)). band = the distance of the sample's pick
    from the nearest boundary between two faces of the cumulative area, as a fraction of the total: a kernel whose cumulative sums
    differ from np.cumsum by less than that picks the same face."""
    v = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    nf = len(f)
    area, ok = face_areas(v, f)
    cdf = np.cumsum(area)
    i = np.arange(n, dtype=np.uint64)
    pick = ((rnd_bits(seed, i, 0) >> _U64(11)).astype(np.float64) * 2.0 ** -53) * cdf[-1]
    raw = np.searchsorted(cdf, pick, side='right')
    face = np.minimum(raw, nf - 1)
    upper = np.where(raw < nf, cdf[face], np.inf)
    lower = np.where(raw > 0, cdf[np.maximum(raw, 1) - 1], -np.inf)
    band = np.minimum(pick - lower, upper - pick) / cdf[-1]
    s = np.float32(2.0 ** -24)
    u1 = (rnd_bits(seed, i, 1) >> _U64(40)).astype(np.float32) * s
    u2 = (rnd_bits(seed, i, 2) >> _U64(40)).astype(np.float32) * s
    fold = (u1 + u2) > np.float32(1)
    u1 = np.where(fold, np.float32(1) - u1, u1)
    u2 = np.where(fold, np.float32(1) - u2, u2)
    fs = np.where(ok[face][:, None], f[face], 0)
    a, b, c = v[fs[:, 0]], v[fs[:, 1]], v[fs[:, 2]]
    pts = (u1[:, None] * (b - a) + u2[:, None] * (c - a)) + a
    pts[~ok[face]] = np.nan
    return pts.astype(np.float32), face.astype(np.int64), band


# ------------------------------------------------------------------------------------------------------------ nearest distance
def nearest_sq_dist_f32(A, B, max_elems=1 << 22):
    """k_nearest restated: float32 ((dx*dx + dy*dy) + dz*dz) on float32 coordinate differences, minimum over B; elementwise float32
    operations only (a matmul or cdist may fuse or reorder), in row chunks of A so that memory stays bounded."""
    A = np.ascontiguousarray(A, np.float32).reshape(-1, 3)
    B = np.ascontiguousarray(B, np.float32).reshape(-1, 3)
    bx, by, bz = (np.ascontiguousarray(B[:, k])[None, :] for k in range(3))
    out = np.empty(len(A), np.float32)
    rows = max(1, max_elems // max(1, len(B)))
    for i0 in range(0, len(A), rows):
        a = A[i0:i0 + rows]
        d = a[:, 0:1] - bx
        np.multiply(d, d, out=d)
        e = a[:, 1:2] - by
        np.multiply(e, e, out=e)
        np.add(d, e, out=d)
        np.subtract(a[:, 2:3], bz, out=e)
        np.multiply(e, e, out=e)
        np.add(d, e, out=d)
        out[i0:i0 + rows] = d.min(1)
    return out
