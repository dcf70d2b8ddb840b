"""Shape evaluation on the MI355X (include/distr_mesh.h, csrc/distr_mesh.hpp): marching cubes, area-weighted surface sampling,
nearest-point distances and the chamfer distance, plus a plain-numpy PLY writer / reader.

What the reference does on the host with scikit-image (marching_cubes_lewiner), plyfile, trimesh (sample_surface) and two scipy
KD-trees (core/evaluation/create_mesh.py, transforms.py, eval_func.py). No third-party package beyond torch and numpy; no CPU path:
every function that computes runs the HIP kernels and raises when there is no device.
"""
import ctypes as C
import threading

import numpy as np
import torch

from distr import binding

_ctxs = {}
_lock = threading.Lock()


def _context(device):
    idx = device.index if device.index is not None else torch.cuda.current_device()
    with _lock:
        if idx not in _ctxs:
            _ctxs[idx] = binding.Context(idx)
        return _ctxs[idx]


def _cuda(x, dtype, device=None):
    """numpy array or tensor -> contiguous CUDA tensor of `dtype` (on `device`, or on the tensor's own / the current device)."""
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(np.ascontiguousarray(x))
    if device is None:
        device = x.device if x.is_cuda else torch.device('cuda', torch.cuda.current_device())
    return x.detach().to(device=device, dtype=dtype).contiguous()


def _workspace(nbytes, device):
    return torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=device)


def _vec3(v):
    a = np.broadcast_to(np.asarray(v, dtype=np.float32), (3,)).copy()
    return (C.c_float * 3)(*[float(x) for x in a])


def marching_cubes(grid, level=0.0, origin=(-1.0, -1.0, -1.0), voxel_size=None):
    """Triangle mesh of the level set {grid == level} of a dense (nx, ny, nz) grid, x slowest (create_sdf_grid's layout); inside =
    value < level. Returns (verts float32 (V, 3), faces int32 (F, 3)) on the grid's device; F = 0 when the level is not crossed.
    Vertex on a sign-changing grid edge: t = a0 / (a0 - a1), a = value - level, coordinate = origin + voxel_size * (index + t) along
    the edge, in float32. voxel_size: a number or one per axis; default 2 / (n - 1) per axis (the grid spans [-1, 1]^3).
    Triangles wind so that right-hand normals point towards increasing values (outwards for an SDF)."""
    g = _cuda(grid, torch.float32)
    if g.dim() != 3:
        raise ValueError('marching_cubes: grid must be 3-D, got shape %s' % (tuple(g.shape),))
    nx, ny, nz = (int(n) for n in g.shape)
    if voxel_size is None:
        voxel_size = [2.0 / (n - 1) if n > 1 else 1.0 for n in (nx, ny, nz)]
    ctx = _context(g.device)
    L = ctx.L
    ws = _workspace(L.distr_mc_workspace_bytes(nx, ny, nz), g.device)
    nv, nf = C.c_int64(), C.c_int64()
    with torch.cuda.device(g.device):
        s = ctx.stream()
        ctx.check(L.distr_mc_count(ctx.h, binding.ptr(g), nx, ny, nz, float(level), C.byref(nv), C.byref(nf), binding.ptr(ws), ws.numel(), s))
        verts = torch.empty((nv.value, 3), dtype=torch.float32, device=g.device)
        faces = torch.empty((nf.value, 3), dtype=torch.int32, device=g.device)
        if nf.value or nv.value:
            ctx.check(L.distr_mc_emit(ctx.h, binding.ptr(g), nx, ny, nz, float(level), _vec3(origin), _vec3(voxel_size),
                                      binding.ptr(verts), nv.value, binding.ptr(faces), nf.value, binding.ptr(ws), ws.numel(), s))
    return verts, faces


def sample_surface(verts, faces, n, seed=0):
    """n points on the mesh, area-weighted (trimesh.sample.sample_surface's rule): returns (points float32 (n, 3), face_index int64
    (n,)) on the mesh's device. The random numbers are a counter-based hash of (seed, sample index): the same seed gives the same
    points."""
    v = _cuda(verts, torch.float32)
    f = _cuda(faces, torch.int32, v.device)
    if v.dim() != 2 or v.shape[1] != 3 or f.dim() != 2 or f.shape[1] != 3:
        raise ValueError('sample_surface: verts (V, 3) and faces (F, 3) expected')
    if f.shape[0] == 0 or v.shape[0] == 0:
        raise ValueError('sample_surface: the mesh has no triangles')
    n = int(n)
    ctx = _context(v.device)
    L = ctx.L
    ws = _workspace(L.distr_sample_workspace_bytes(f.shape[0]), v.device)
    pts = torch.empty((n, 3), dtype=torch.float32, device=v.device)
    fidx = torch.empty((n,), dtype=torch.int32, device=v.device)
    with torch.cuda.device(v.device):
        ctx.check(L.distr_sample_surface(ctx.h, binding.ptr(v), v.shape[0], binding.ptr(f), f.shape[0], n, int(seed) & (2 ** 64 - 1),
                                         binding.ptr(pts), binding.ptr(fidx), binding.ptr(ws), ws.numel(), ctx.stream()))
    return pts, fidx.long()


def _nearest(a, b, sums=False):
    A = _cuda(a, torch.float32).reshape(-1, 3)
    B = _cuda(b, torch.float32, A.device).reshape(-1, 3)
    if B.shape[0] == 0:
        raise ValueError('nearest distance to an empty point set')
    ctx = _context(A.device)
    L = ctx.L
    ws = _workspace(L.distr_nearest_workspace_bytes(A.shape[0]), A.device)
    d2 = torch.empty((A.shape[0],), dtype=torch.float32, device=A.device)
    out = torch.zeros((2,), dtype=torch.float64, device=A.device) if sums else None
    with torch.cuda.device(A.device):
        ctx.check(L.distr_nearest_sqdist(ctx.h, binding.ptr(A), A.shape[0], binding.ptr(B), B.shape[0], binding.ptr(d2), binding.ptr(out),
                                         binding.ptr(ws), ws.numel(), ctx.stream()))
    return d2, out


def nearest_sq_dist(a, b):
    """(na,) float32: squared distance from every point of a (na, 3) to its nearest point of b (nb, 3). Brute force over all pairs
    with float32 coordinate differences (not the |a|^2 + |b|^2 - 2ab expansion, which cancels for close points)."""
    return _nearest(a, b)[0]


def chamfer(p1, p2, use_square_dist=True, separate=False):
    """The reference's compute_chamfer_distance (eval_func.py:5-25): mean over p2 of the distance to the nearest point of p1 plus
    the same the other way round, squared distances unless use_square_dist=False. separate=True: the two squared means
    (compute_chamfer_distance_separate, :27-41). numpy arrays or CUDA tensors in, numpy float64 out; means accumulated in float64."""
    n1, n2 = len(p1), len(p2)
    if n1 == 0 or n2 == 0:
        raise ValueError('chamfer distance of an empty point set')
    _, s21 = _nearest(p2, p1, sums=True)
    _, s12 = _nearest(p1, p2, sums=True)
    s21, s12 = s21.cpu().numpy(), s12.cpu().numpy()
    k = 0 if (use_square_dist or separate) else 1
    d21, d12 = np.float64(s21[k] / n2), np.float64(s12[k] / n1)
    if separate:
        return d21, d12
    return d21 + d12


# --------------------------------------------------------------------------------------------------------------------------- PLY
_PLY_TYPES = {'char': 'i1', 'int8': 'i1', 'uchar': 'u1', 'uint8': 'u1', 'short': 'i2', 'int16': 'i2', 'ushort': 'u2', 'uint16': 'u2',
              'int': 'i4', 'int32': 'i4', 'uint': 'u4', 'uint32': 'u4', 'float': 'f4', 'float32': 'f4', 'double': 'f8', 'float64': 'f8'}


def write_ply(fname, verts, faces):
    """Binary little-endian PLY with plyfile's default layout for what convert_sdf_samples_to_ply writes (create_mesh.py:187-201):
    vertex `float x, y, z`, face `property list uchar int vertex_indices`."""
    v = np.ascontiguousarray(verts.detach().cpu().numpy() if torch.is_tensor(verts) else verts, dtype='<f4').reshape(-1, 3)
    f = np.asarray(faces.detach().cpu().numpy() if torch.is_tensor(faces) else faces).reshape(-1, 3)
    header = ('ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n'
              'element face %d\nproperty list uchar int vertex_indices\nend_header\n' % (len(v), len(f)))
    rec = np.empty(len(f), dtype=[('n', 'u1'), ('i', '<i4', (3,))])
    rec['n'] = 3
    rec['i'] = f
    with open(fname, 'wb') as out:
        out.write(header.encode('ascii'))
        out.write(v.tobytes())
        out.write(rec.tobytes())


def read_ply(fname):
    """(verts float32 (V, 3), faces int32 (F, 3)) of a binary little-endian PLY with a vertex element (x, y, z among fixed-size
    properties) and a triangle face element (one list property of vertex indices)."""
    with open(fname, 'rb') as f:
        data = f.read()
    end = data.find(b'end_header\n')
    if not data.startswith(b'ply\n') or end < 0:
        raise ValueError('%s: not a PLY file' % fname)
    lines = data[:end].decode('ascii').splitlines()
    body = memoryview(data)[end + len(b'end_header\n'):]
    if 'format binary_little_endian 1.0' not in [l.strip() for l in lines]:
        raise ValueError('%s: only binary_little_endian PLY files are read' % fname)
    elems = []
    for l in lines:
        w = l.split()
        if not w:
            continue
        if w[0] == 'element':
            elems.append((w[1], int(w[2]), []))
        elif w[0] == 'property':
            elems[-1][2].append(tuple(w[1:]))
    verts, faces, off = None, None, 0
    for name, count, props in elems:
        if any(p[0] == 'list' for p in props):
            if name != 'face' or len(props) != 1:
                raise ValueError('%s: list properties are read only as the single property of a face element' % fname)
            _, ct, it, _ = props[0]
            dt = np.dtype([('n', '<' + _PLY_TYPES[ct]), ('i', '<' + _PLY_TYPES[it], (3,))])
            rec = np.frombuffer(body, dtype=dt, count=count, offset=off)
            if count and not (rec['n'] == 3).all():
                raise ValueError('%s: faces other than triangles' % fname)
            faces = rec['i'].astype(np.int32)
            off += dt.itemsize * count
        else:
            dt = np.dtype([(p[1], '<' + _PLY_TYPES[p[0]]) for p in props])
            rec = np.frombuffer(body, dtype=dt, count=count, offset=off)
            if name == 'vertex':
                verts = np.stack([rec['x'], rec['y'], rec['z']], 1).astype(np.float32)
            off += dt.itemsize * count
    if verts is None:
        raise ValueError('%s: no vertex element' % fname)
    return verts, (faces if faces is not None else np.zeros((0, 3), np.int32))
