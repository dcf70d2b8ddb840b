"""Shape evaluation on the MI355X (include/distr_mesh.h, csrc/distr_mesh.hpp): marching cubes, area-weighted surface sampling,
nearest-point distances and the chamfer distance, plus a plain-numpy PLY writer / reader; and the way back from a mesh to training
data: signed distances to a triangle mesh and DeepSDF-style SDF samples (signed_distance, sdf_samples, the pos / neg npz layout); and
from a mesh to images: depth, normal and mask maps in the renderer's camera convention (render_mesh).

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


# ------------------------------------------------------------------------------------------------- SDF samples from a mesh
SDF_CHUNK = 1024                  # faces per chunk of distr_mesh_sdf (SDF_CHUNK of csrc/distr_mesh.hpp): one float64 per query and chunk
_SDF_WS_BYTES = 64 << 20          # signed_distance takes its queries in pieces whose workspace stays below this


def signed_distance(verts, faces, points, details=False):
    """Signed distance of points (Q, 3) to the triangle mesh, float32 (Q,) on the mesh's device: the distance to the closest point of
    the nearest triangle (exact point-to-triangle distance in float32, brute force over all pairs), negative where the generalised
    winding number w says inside (|w| > 0.5; w = +1 inside a closed mesh wound like marching_cubes' output, 0 outside, fractional for
    an open one). details=True: (sdf, squared distance, w float32, nearest face int64 -- the lowest index among equal distances).
    Triangles that name a vertex outside the array, have a coordinate that is not finite or a float32 cross product of exactly zero
    are skipped; with no triangle left the distance is +inf and the face -1. A point with a coordinate that is not finite gives NaN
    and face -1. The queries are processed in pieces so that the workspace stays bounded; every row depends on its own point only."""
    v = _cuda(verts, torch.float32)
    f = _cuda(faces, torch.int32, v.device)
    if v.dim() != 2 or v.shape[1] != 3 or f.dim() != 2 or f.shape[1] != 3:
        raise ValueError('signed_distance: verts (V, 3) and faces (F, 3) expected')
    if f.shape[0] == 0 or v.shape[0] == 0:
        raise ValueError('signed_distance: the mesh has no triangles')
    q = _cuda(points, torch.float32, v.device).reshape(-1, 3)
    nq, nf = q.shape[0], f.shape[0]
    ctx = _context(v.device)
    L = ctx.L
    sdf = torch.empty((nq,), dtype=torch.float32, device=v.device)
    d2 = torch.empty((nq,), dtype=torch.float32, device=v.device) if details else None
    w = torch.empty((nq,), dtype=torch.float32, device=v.device) if details else None
    fidx = torch.empty((nq,), dtype=torch.int32, device=v.device) if details else None
    nchunks = (nf + SDF_CHUNK - 1) // SDF_CHUNK
    piece = max(256, min(1 << 16, _SDF_WS_BYTES // (8 * (nchunks + 1))) // 256 * 256)
    ws = _workspace(L.distr_mesh_sdf_workspace_bytes(min(piece, max(nq, 1)), nf), v.device)
    with torch.cuda.device(v.device):
        s = ctx.stream()
        for i0 in range(0, nq, piece):
            n = min(piece, nq - i0)
            ctx.check(L.distr_mesh_sdf(ctx.h, binding.ptr(v), v.shape[0], binding.ptr(f), nf, binding.ptr(q[i0:]), n, binding.ptr(sdf[i0:]),
                                       binding.ptr(d2[i0:]) if details else None, binding.ptr(w[i0:]) if details else None,
                                       binding.ptr(fidx[i0:]) if details else None, binding.ptr(ws), ws.numel(), s))
    if details:
        return sdf, d2, w, fidx.long()
    return sdf


def sdf_queries(surface_points, sigmas, n_uniform, half_extent=1.0, seed=0):
    """DeepSDF-style query points (2 * S + n_uniform, 3) float32 from S surface points: rows 2 i and 2 i + 1 are point i plus
    sigmas[0] resp. sigmas[1] times standard normals, the last n_uniform rows are uniform in [-half_extent, half_extent)^3. Every row
    is a function of (seed, its index) alone."""
    p = _cuda(surface_points, torch.float32).reshape(-1, 3)
    ns, nu = p.shape[0], int(n_uniform)
    if nu < 0:
        raise ValueError('sdf_queries: n_uniform must not be negative')
    ctx = _context(p.device)
    out = torch.empty((2 * ns + nu, 3), dtype=torch.float32, device=p.device)
    with torch.cuda.device(p.device):
        ctx.check(ctx.L.distr_sdf_queries(ctx.h, binding.ptr(p), ns, float(sigmas[0]), float(sigmas[1]), nu, float(half_extent),
                                          int(seed) & (2 ** 64 - 1), binding.ptr(out), ctx.stream()))
    return out


def sdf_samples(verts, faces, n_surface, seed=0, sigmas=(0.005 ** 0.5, 0.0005 ** 0.5), n_uniform=None, half_extent=1.0):
    """SDF training samples of a mesh, the input of decode_sdf_train: n_surface area-weighted surface points (sample_surface), each
    perturbed twice (standard deviations `sigmas`), plus n_uniform points uniform in [-half_extent, half_extent)^3 (default
    n_surface // 10), all with their signed distance. Returns {'pos': (Np, 4), 'neg': (Nn, 4)} float32 on the mesh's device, rows
    (x, y, z, sdf), split by sign (pos: sdf >= 0) in query order; Np + Nn = 2 * n_surface + n_uniform less the queries whose distance
    is NaN (none for a mesh with finite vertices). The defaults follow the recipe DeepSDF published for its preprocessing (variances
    0.005 and 0.0005 in the unit sphere); they are parameters, and nothing here reproduces that program's samples."""
    n_surface = int(n_surface)
    if n_uniform is None:
        n_uniform = n_surface // 10
    pts, _ = sample_surface(verts, faces, n_surface, seed=seed)
    q = sdf_queries(pts, sigmas, n_uniform, half_extent, seed)
    sdf = signed_distance(verts, faces, q)
    rows = torch.cat([q, sdf[:, None]], 1)
    return {'pos': rows[sdf >= 0], 'neg': rows[sdf < 0]}


# ------------------------------------------------------------------------------------------------- images of a mesh
RENDER_TILE = 256                 # face records per LDS tile of distr_mesh_render (RC_TILE of csrc/distr_mesh.hpp)
RENDER_CHUNK = 1024               # faces per chunk (RC_CHUNK): the chunks' nearest hits meet in an integer atomic min
RENDER_BLOCK = 512                # pixels per block of k_mesh_cast (MB * RC_PPT)
_MAX_VIEWS = binding.MAX_VIEWS    # views per distr_mesh_render call; more go in pieces


def render_mesh(verts, faces, intrinsic, RT, img_hw, transform_matrix=None, normal_frame='image', details=False):
    """Depth, normal and mask maps of a triangle mesh in the renderer's camera convention: what SDFRenderer.render returns for a
    decoder, for a mesh -- a ground-truth shape, a scan, the output of marching_cubes. intrinsic (3, 3), RT (3, 4) = [R | T] or
    (B, 3, 4) for any B (more than 64 views go in pieces, byte for byte the same), img_hw (H, W), transform_matrix (3, 3) as
    SDFRenderer's (default: the renderer's [[1, 0, 0], [0, 0, -1], [0, 1, 0]]).
    Returns (depth float32 (H, W), normal float32 (H, W, 3), mask uint8 (H, W)) on the mesh's device, with a leading B for a batch:
    depth = ray parameter t times calib_map (render's depth; 1e11 where no triangle is hit), normal = the hit triangle's geometric
    normal oriented towards the camera whatever the winding (0 for a miss) -- normal_frame='image': R (M n) with x negated, the
    convention of render's normals; 'world': M n, what SDFRenderer_deepsdf.get_samples expects. details=True: also zdepth (t; 1e11 for a
    miss), face (int64, -1 for a miss: the lowest index among equally near triangles) and bary (H, W, 2), the weights of the hit
    triangle's second and third corner.
    Brute force over all (ray, triangle) pairs in float32 with edge functions that are exact negatives of each other on a shared edge:
    a closed indexed mesh has no holes along its edges. Not differentiable: the maps are observations. Triangles that name a vertex
    outside the array, have a coordinate that is not finite or a float32 cross product of exactly zero are skipped; a view whose RT is
    not finite sees nothing."""
    v = _cuda(verts, torch.float32)
    f = _cuda(faces, torch.int32, v.device)
    if v.dim() != 2 or v.shape[1] != 3 or f.dim() != 2 or f.shape[1] != 3:
        raise ValueError('render_mesh: verts (V, 3) and faces (F, 3) expected')
    if f.shape[0] == 0 or v.shape[0] == 0:
        raise ValueError('render_mesh: the mesh has no triangles')
    if normal_frame not in binding.MESH_NORMAL_FRAMES:
        raise ValueError("render_mesh: normal_frame %r: 'image' or 'world'" % (normal_frame,))
    rt = _cuda(RT, torch.float32, v.device)
    if tuple(rt.shape) != (3, 4) and (rt.dim() != 3 or tuple(rt.shape[1:]) != (3, 4) or rt.shape[0] == 0):
        raise ValueError('render_mesh: RT has shape %s; (3, 4) or (B, 3, 4) expected' % (tuple(rt.shape),))
    single = rt.dim() == 2
    rt = rt.reshape(-1, 3, 4)
    if torch.is_tensor(intrinsic):
        intrinsic = intrinsic.detach().cpu().numpy()
    if transform_matrix is None:
        transform_matrix = np.array([[1., 0., 0.], [0., 0., -1.], [0., 1., 0.]])       # SDFRenderer's default
    elif torch.is_tensor(transform_matrix):
        transform_matrix = transform_matrix.detach().cpu().numpy()
    if np.asarray(intrinsic).shape != (3, 3) or np.asarray(transform_matrix).shape != (3, 3):
        raise ValueError('render_mesh: intrinsic and transform_matrix are (3, 3)')
    H, W = int(img_hw[0]), int(img_hw[1])
    if H < 1 or W < 1 or H * W * min(rt.shape[0], _MAX_VIEWS) >= 2 ** 31:
        raise ValueError('render_mesh: image size %d x %d' % (H, W))
    cfg = binding.make_mesh_render_cfg((H, W), intrinsic, transform_matrix, normal_frame)
    B, dev = rt.shape[0], v.device
    ctx = _context(dev)
    L = ctx.L
    depth = torch.empty((B, H, W), dtype=torch.float32, device=dev)
    normal = torch.empty((B, H, W, 3), dtype=torch.float32, device=dev)
    mask = torch.empty((B, H, W), dtype=torch.uint8, device=dev)
    zdepth = torch.empty((B, H, W), dtype=torch.float32, device=dev) if details else None
    face = torch.empty((B, H, W), dtype=torch.int32, device=dev) if details else None
    bary = torch.empty((B, H, W, 2), dtype=torch.float32, device=dev) if details else None
    ws = _workspace(L.distr_mesh_render_workspace_bytes(H, W, min(B, _MAX_VIEWS)), dev)
    with torch.cuda.device(dev):
        s = ctx.stream()
        for b0 in range(0, B, _MAX_VIEWS):
            n = min(_MAX_VIEWS, B - b0)
            ctx.check(L.distr_mesh_render(ctx.h, C.byref(cfg), binding.ptr(v), v.shape[0], binding.ptr(f), f.shape[0], n, binding.ptr(rt[b0:]),
                                          binding.ptr(depth[b0:]), binding.ptr(zdepth[b0:]) if details else None, binding.ptr(normal[b0:]),
                                          binding.ptr(mask[b0:]), binding.ptr(face[b0:]) if details else None,
                                          binding.ptr(bary[b0:]) if details else None, binding.ptr(ws), ws.numel(), s))
    out = (depth, normal, mask) + ((zdepth, face.long(), bary) if details else ())
    return tuple(o[0] for o in out) if single else out


def write_sdf_npz(fname, samples):
    """DeepSDF's sample file: an npz with float32 arrays 'pos' and 'neg' of rows (x, y, z, sdf)."""
    arrs = {k: np.ascontiguousarray(samples[k].detach().cpu().numpy() if torch.is_tensor(samples[k]) else samples[k], dtype=np.float32).reshape(-1, 4)
            for k in ('pos', 'neg')}
    with open(fname, 'wb') as out:
        np.savez(out, **arrs)


def read_sdf_npz(fname):
    """{'pos': (Np, 4), 'neg': (Nn, 4)} float32 numpy arrays of a file written by write_sdf_npz (or by DeepSDF's preprocessing)."""
    with np.load(fname) as z:
        return {k: np.ascontiguousarray(z[k], dtype=np.float32).reshape(-1, 4) for k in ('pos', 'neg')}


def normalize_to_unit_sphere(verts, buffer=1.03):
    """(verts', offset, scale) with verts' = (verts + offset) * scale: the bounding box's centre moved to the origin and the farthest
    vertex to radius 1 / buffer. offset (3,) and scale are float64; the convention is the one the reference's loaders apply to cameras
    and depth maps with normalization_params['offset'] / ['scale']. verts' is float32, a tensor on the input's device for a tensor."""
    v = verts.detach().cpu().numpy() if torch.is_tensor(verts) else np.asarray(verts)
    v = v.reshape(-1, 3)
    if len(v) == 0:
        raise ValueError('normalize_to_unit_sphere: no vertices')
    v64 = v.astype(np.float64)
    offset = -(v.max(0).astype(np.float64) + v.min(0).astype(np.float64)) / 2
    r = np.sqrt(((v64 + offset) ** 2).sum(1).max())
    if not np.isfinite(r) or r == 0:
        raise ValueError('normalize_to_unit_sphere: vertices that are not finite, or a single point')
    scale = 1.0 / (r * float(buffer))
    out = ((v64 + offset) * scale).astype(np.float32)
    if torch.is_tensor(verts):
        out = torch.from_numpy(out).to(verts.device)
    return out, offset, scale


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
