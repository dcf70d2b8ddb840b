"""numpy restatement of the mesh render kernels (csrc/distr_mesh.hpp: k_mesh_cast / k_mesh_finish) for tests/test_mesh_render_host.py
and tests/test_gpu_mesh_render.py.

`render` restates the kernels in float32, in the operation order their header comment spells out: elementwise float32 operations only
(numpy neither fuses nor reorders them; its division and square root are correctly rounded like the build's), so every output comes out
bit for bit. `render64` is written on its own -- matrix products, np.cross, float64 throughout, from the same float32 inputs -- and
applies the same hit rule: the yardstick the float32 results are measured against. The skip rule is the kernel's in both (the float32
cross product decides, mesh_sdf_restatement.face_records).

Both return a dict of (H, W[, k]) arrays for ONE view: depth, zdepth, normal, mask (uint8), face (int32, -1 for a miss), bary, and
nhits = the number of triangles each ray hits (the nearest of them is the one reported)."""
import numpy as np

from mesh_sdf_restatement import face_records

RENDER_TILE = 256                  # RC_TILE
RENDER_CHUNK = 1024                # RC_CHUNK
RENDER_BLOCK = 512                 # MB * RC_PPT: pixels per block of k_mesh_cast
MB = 256                           # pixels per block of k_mesh_finish
MISS = 1e11
M_DEFAULT = np.array([[1, 0, 0], [0, 0, -1], [0, 1, 0]], np.float32)       # the renderer's transform_matrix
_NONE = np.uint64(0x7f800000ffffffff)
_F = np.float32


def k_inv(intrinsic):
    """float32(inv(K)) as SDFRenderer forms the K_inv it hands to the library."""
    return np.linalg.inv(np.asarray(intrinsic, dtype=np.float64)).astype(np.float32)


def _dot(u, v):
    return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]


def _cross(p, q):
    return [p[1] * q[2] - p[2] * q[1], p[2] * q[0] - p[0] * q[2], p[0] * q[1] - p[1] * q[0]]


def camera(K_inv, M, RT, H, W):
    """float32, the kernel's order: (o [3 scalars], e [3 arrays (P,)], calib (P,), R (3, 3)). o = M^T c with c = -R^T T as k_prep forms
    it, e = M^T d with d of make_ray at the integer pixel centres."""
    Ki, M, RT = (np.asarray(x, np.float32) for x in (K_inv, M, RT))
    R, T = RT[:, :3], RT[:, 3]
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        c = [-(R[0, i] * T[0] + R[1, i] * T[1] + R[2, i] * T[2]) for i in range(3)]
        o = [M[0, i] * c[0] + M[1, i] * c[1] + M[2, i] * c[2] for i in range(3)]
        pix = np.arange(H * W)
        x, y = (pix % W).astype(_F), (pix // W).astype(_F)
        h = [Ki[a, 0] * x + Ki[a, 1] * y + Ki[a, 2] for a in range(3)]
        hn = np.sqrt(h[0] * h[0] + h[1] * h[1] + h[2] * h[2])
        calib = h[2] / (hn + _F(1e-12))
        r = [R[0, i] * h[0] + R[1, i] * h[1] + R[2, i] * h[2] for i in range(3)]
        rn = np.sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2])
        d = [r[i] / (rn + _F(1e-12)) for i in range(3)]
        e = [M[0, i] * d[0] + M[1, i] * d[1] + M[2, i] * d[2] for i in range(3)]
    assert all(a.dtype == _F for a in e + o + [calib])
    return o, e, calib, R


def _corners(verts, faces, RT):
    """a, b, c (F, 3) float32 of every face (index 0 where it names a vertex outside the array) and counted (F,)."""
    v = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    inr = ((f >= 0) & (f < len(v))).all(1)
    fs = np.where(inr[:, None], f, 0)
    counted = face_records(v, f)[3] & bool(np.isfinite(np.asarray(RT, np.float32)).all())
    return v[fs[:, 0]], v[fs[:, 1]], v[fs[:, 2]], counted


def _rel(a, b, c, o, sel=slice(None)):
    """A, B, C as lists of three component arrays: the corners `sel` relative to the camera."""
    return tuple([p[sel, k] - o[k] for k in range(3)] for p in (a, b, c))


def _uvw(e, A, B, C):
    Na, Nb, Nc = _cross(C, B), _cross(A, C), _cross(B, A)
    return _dot(e, Na), _dot(e, Nb), _dot(e, Nc)


def _t(e, A, B, C):
    Ng = _cross([B[k] - A[k] for k in range(3)], [C[k] - A[k] for k in range(3)])
    den = _dot(e, Ng)
    return _dot(A, Ng) / den, Ng, den


def _mixed(U, V, W):
    return ((U < 0) | (V < 0) | (W < 0)) & ((U > 0) | (V > 0) | (W > 0))


def render(verts, faces, K_inv, M, RT, H, W, normal_frame='image', max_elems=1 << 22):
    P = H * W
    o, e, calib, R = camera(K_inv, M, RT, H, W)
    M = np.asarray(M, np.float32)
    a, b, c, counted = _corners(verts, faces, RT)
    nf = len(a)
    zero = np.zeros_like(a)
    az, bz, cz = (np.where(counted[:, None], p, zero) for p in (a, b, c))          # skipped faces: no NaN noise, masked below
    best = np.full(P, _NONE, np.uint64)
    nhits = np.zeros(P, np.int64)
    rows = max(1, max_elems // max(1, nf))
    with np.errstate(invalid='ignore', over='ignore', divide='ignore', under='ignore'):
        A, B, C = _rel(az, bz, cz, o)
        A_, B_, C_ = ([x[None, :] for x in p] for p in (A, B, C))
        for i0 in range(0, P, rows):
            eb = [x[i0:i0 + rows, None] for x in e]
            U, V, Wd = _uvw(eb, A_, B_, C_)
            det = (U + V) + Wd
            assert det.dtype == _F
            pi, fi = np.nonzero(counted[None, :] & ~_mixed(U, V, Wd) & (det != 0))
            ep = [x[i0 + pi] for x in e]
            t, _, _ = _t(ep, *_rel(a, b, c, o, fi))
            hit = np.isfinite(t) & (t > 0)
            key = (t[hit].view(np.uint32).astype(np.uint64) << np.uint64(32)) | fi[hit].astype(np.uint64)
            np.minimum.at(best, i0 + pi[hit], key)
            np.add.at(nhits, i0 + pi[hit], 1)
        # k_mesh_finish
        px = np.nonzero(best != _NONE)[0]
        fw = (best[px] & np.uint64(0xffffffff)).astype(np.int64)
        ep = [x[px] for x in e]
        A, B, C = _rel(a, b, c, o, fw)
        U, V, Wd = _uvw(ep, A, B, C)
        det = (U + V) + Wd
        t, Ng, den = _t(ep, A, B, C)
        assert np.array_equal(t.view(np.uint32), (best[px] >> np.uint64(32)).astype(np.uint32))
        ln = np.sqrt(_dot(Ng, Ng))
        g = [np.where(den > 0, -Ng[k], Ng[k]) / ln + _F(0) for k in range(3)]
        n = [M[k, 0] * g[0] + M[k, 1] * g[1] + M[k, 2] * g[2] for k in range(3)]
        if normal_frame == 'image':
            n = [R[k, 0] * n[0] + R[k, 1] * n[1] + R[k, 2] * n[2] for k in range(3)]
            n[0] = -n[0]
        else:
            assert normal_frame == 'world'
        out = {'depth': np.full(P, MISS, _F), 'zdepth': np.full(P, MISS, _F), 'normal': np.zeros((P, 3), _F), 'mask': np.zeros(P, np.uint8),
               'face': np.full(P, -1, np.int32), 'bary': np.zeros((P, 2), _F), 'nhits': nhits}
        out['zdepth'][px], out['depth'][px] = t, t * calib[px]
        out['normal'][px] = np.stack(n, 1)
        out['bary'][px] = np.stack([V / det, Wd / det], 1)
        out['mask'][px], out['face'][px] = 1, fw
    assert all(out[k].dtype == _F for k in ('depth', 'zdepth', 'normal', 'bary'))
    return {k: x.reshape((H, W) + x.shape[1:]) for k, x in out.items()}


def edge_functions(verts, faces, K_inv, M, RT, H, W, pix, face):
    """(U, V, W) float32 of the pair (pixel index `pix`, face `face`) as the kernel forms them."""
    o, e, _, _ = camera(K_inv, M, RT, H, W)
    a, b, c, _ = _corners(verts, faces, RT)
    return tuple(_F(x[0]) for x in _uvw([x[[pix]] for x in e], *_rel(a, b, c, o, [face])))


def camera64(K_inv, M, RT, H, W):
    """float64 from the same float32 inputs: (o (3,), e (P, 3), calib (P,), R (3, 3))."""
    Ki, M, RT = (np.asarray(x, np.float32).astype(np.float64) for x in (K_inv, M, RT))
    R, T = RT[:, :3], RT[:, 3]
    pix = np.arange(H * W)
    h = np.stack([pix % W, pix // W, np.ones_like(pix)], 1).astype(np.float64) @ Ki.T
    calib = h[:, 2] / (np.linalg.norm(h, axis=1) + 1e-12)
    r = h @ R                                                  # rows R^T h
    d = r / (np.linalg.norm(r, axis=1, keepdims=True) + 1e-12)
    return M.T @ (-R.T @ T), d @ M, calib, R


def render64(verts, faces, K_inv, M, RT, H, W, normal_frame='image', max_elems=1 << 22):
    P = H * W
    with np.errstate(invalid='ignore'):
        o, e, calib, R = camera64(K_inv, M, RT, H, W)
    M = np.asarray(M, np.float32).astype(np.float64)
    a, b, c, counted = _corners(verts, faces, RT)
    idx = np.nonzero(counted)[0]
    A, B, C = (p[idx].astype(np.float64) - o for p in (a, b, c))
    N3 = np.stack([np.cross(C, B), np.cross(A, C), np.cross(B, A)])                # (3, F', 3)
    Ng = np.cross(B - A, C - A)
    out = {'depth': np.full(P, MISS), 'zdepth': np.full(P, MISS), 'normal': np.zeros((P, 3)), 'mask': np.zeros(P, np.uint8),
           'face': np.full(P, -1, np.int32), 'bary': np.zeros((P, 2)), 'nhits': np.zeros(P, np.int64)}
    rows = max(1, max_elems // max(1, len(idx)))
    for i0 in range(0, P if len(idx) else 0, rows):
        eb = e[i0:i0 + rows]
        UVW = np.einsum('pk,jfk->jpf', eb, N3)
        det = UVW.sum(0)
        mixed = (UVW < 0).any(0) & (UVW > 0).any(0)
        with np.errstate(invalid='ignore', divide='ignore'):
            t = (A * Ng).sum(1)[None, :] / (eb @ Ng.T)
        t = np.where(~mixed & (det != 0) & np.isfinite(t) & (t > 0), t, np.inf)
        out['nhits'][i0:i0 + rows] = np.isfinite(t).sum(1)
        j = t.argmin(1)                                          # the first of equal minima: the lowest face
        p = np.nonzero(np.isfinite(t.min(1)))[0]
        j = j[p]
        n = Ng[j] * -np.sign((eb[p] * Ng[j]).sum(1))[:, None] / np.linalg.norm(Ng[j], axis=1, keepdims=True)
        n = n @ M.T
        if normal_frame == 'image':
            n = (n @ R.T) * [-1.0, 1.0, 1.0]
        out['zdepth'][i0 + p], out['depth'][i0 + p] = t[p, j], t[p, j] * calib[i0 + p]
        out['normal'][i0 + p], out['mask'][i0 + p], out['face'][i0 + p] = n, 1, idx[j]
        out['bary'][i0 + p] = np.stack([UVW[1, p, j] / det[p, j], UVW[2, p, j] / det[p, j]], 1)
    return {k: x.reshape((H, W) + x.shape[1:]) for k, x in out.items()}


# ------------------------------------------------------------------------------------------------------------ test cameras
def look_at(eye, target=(0.0, 0.0, 0.0), roll_deg=0.0):
    """RT (3, 4) float32 of a camera at `eye` (world frame) looking at `target`: rows of R = the camera's x, y, z axes, T = -R eye."""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    z = target - eye
    z /= np.linalg.norm(z)
    up = np.array([0.0, 0.0, 1.0]) if abs(z[2]) < 0.9 else np.array([0.0, 1.0, 0.0])
    x = np.cross(z, up)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    a = np.deg2rad(roll_deg)
    x, y = np.cos(a) * x + np.sin(a) * y, -np.sin(a) * x + np.cos(a) * y
    R = np.stack([x, y, z])
    return np.concatenate([R, (-R @ eye)[:, None]], 1).astype(np.float32)


def intrinsic(H, W, f=None, cx=None, cy=None):
    f = 1.2 * max(H, W) if f is None else f
    return np.array([[f, 0, (W - 1) / 2 if cx is None else cx], [0, f, (H - 1) / 2 if cy is None else cy], [0, 0, 1]], np.float64)
