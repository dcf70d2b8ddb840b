"""numpy float32 restatement of the GPU marching cubes (csrc/distr_mesh.hpp: k_mc_classify / k_mc_compact / k_mc_faces), read from
the same table, for tests/test_gpu_mesh.py. Vertices: one per sign-changing grid edge, ordered by (owning grid point, axis x < y < z),
t = a0 / (a0 - a1) with a = value - level and coord = origin + voxel_size * (index + t), in float32 without fused multiply-adds; faces
ordered by (cell = its lowest corner, table order)."""
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
