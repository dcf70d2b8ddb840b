"""CPU-only checks of the mesh render feature: the new part of the mesh C ABI against the binding, and the numpy restatement
(tests/mesh_render_restatement.py) that tests/test_gpu_mesh_render.py compares the kernels with, validated here against independent
statements: the analytic ray-sphere depth on marching-cubes spheres, the float64 evaluation of the same rule, watertightness (every
ray of a closed mesh hits an even number of triangles, no hole inside the silhouette), constructed rays through a shared edge and
through a vertex, and the hit and skip rules."""
import functools
import os

import numpy as np
import pytest

from conftest import ROOT
import mesh_render_restatement as Q
import mesh_restatement as R
import mesh_sdf_restatement as S

CENTER, RADIUS = (0.03, -0.02, 0.01), 0.5


def test_render_abi_exported_and_constants():
    import ctypes as C
    from distr import binding, mesh
    for name in ('distr_mesh_render_workspace_bytes', 'distr_mesh_render'):
        assert name in binding.MESH_EXPORTS
    hdr = open(os.path.join(ROOT, 'include', 'distr_mesh.h')).read()
    assert 'distr_mesh_render(' in hdr and 'distr_mesh_render_cfg' in hdr
    src = open(os.path.join(ROOT, 'dist-renderer_amd', 'csrc', 'distr_mesh.hpp')).read()
    for name, val in (('RC_TILE', mesh.RENDER_TILE), ('RC_CHUNK', mesh.RENDER_CHUNK)):
        assert 'constexpr int %s = %d;' % (name, val) in src
    assert (mesh.RENDER_TILE, mesh.RENDER_CHUNK, mesh.RENDER_BLOCK) == (Q.RENDER_TILE, Q.RENDER_CHUNK, Q.RENDER_BLOCK)
    assert C.sizeof(binding.MeshRenderCfg) == 4 + 8 + 36 + 36 + 4
    binding.build_library()
    L = binding.lib()
    ws = L.distr_mesh_render_workspace_bytes
    assert ws(0, 4, 1) == 0 and ws(4, 4, 0) == 0 and ws(4, 4, 65) == 0 and ws(1 << 16, 1 << 15, 1) == 0       # H * W * nviews = 2^31
    assert ws(16, 16, 2) - ws(16, 16, 1) == 256 * 8                  # one 64-bit key per pixel and view
    assert L.distr_mesh_render(None, None, None, 0, None, 0, 0, None, None, None, None, None, None, None, None, 0, None) == -1
    cfg = binding.make_mesh_render_cfg((3, 5), Q.intrinsic(3, 5), Q.M_DEFAULT, 'world')
    assert (cfg.H, cfg.W, cfg.normal_frame, cfg.struct_size) == (3, 5, 0, C.sizeof(binding.MeshRenderCfg))
    assert np.array_equal(np.array(cfg.K_inv[:], np.float32).reshape(3, 3), Q.k_inv(Q.intrinsic(3, 5)))


@functools.lru_cache(maxsize=None)
def _sphere(N):
    """The marching-cubes sphere of an N^3 grid under a rotated off-centre camera: (verts, faces, K_inv, RT, H, W, float32 render,
    float64 render)."""
    v, f = R.marching_cubes(R.sphere_grid(N, CENTER, RADIUS))
    assert (R.edge_use_counts(f) == 2).all() and R.euler(v, f) == 2
    H, W = (48, 40) if N == 16 else (48, 48)
    Ki = Q.k_inv(Q.intrinsic(H, W, f=2.1 * W, cx=0.45 * W, cy=0.55 * H))
    RT = Q.look_at(Q.M_DEFAULT.astype(np.float64) @ np.array([1.4, -1.9, 0.8]), Q.M_DEFAULT.astype(np.float64) @ np.array([0.1, 0.0, -0.05]), roll_deg=25)
    return v, f, Ki, RT, H, W, Q.render(v, f, Ki, Q.M_DEFAULT, RT, H, W), Q.render64(v, f, Ki, Q.M_DEFAULT, RT, H, W)


SPHERES = (16, 32)


@pytest.mark.parametrize('N', SPHERES)
def test_float32_depth_is_the_analytic_sphere_depth(N):
    """Vertices sit on linearly interpolated grid values (off the sphere by at most h^2 / (8 r)), a chord of length h * sqrt(3) sags
    3 h^2 / (8 r) below the sphere, seen along the ray that is divided by the cosine of the incidence: within h^2 / r for cos >= 0.5."""
    v, f, Ki, RT, H, W, r32, _ = _sphere(N)
    o, e, calib, _ = Q.camera64(Ki, Q.M_DEFAULT, RT, H, W)
    oc = o - np.array(CENTER)
    bq = e @ oc
    disc = bq * bq - (oc @ oc - RADIUS ** 2)
    with np.errstate(invalid='ignore'):
        t = -bq - np.sqrt(disc)
    nrm = (oc + t[:, None] * e) / RADIUS
    with np.errstate(invalid='ignore'):
        sel = ((disc > 0) & (-(nrm * e).sum(1) >= 0.5)).reshape(H, W)
    assert sel.sum() > 200
    assert (r32['mask'][sel] == 1).all()
    h = 2.0 / (N - 1)
    err = np.abs(r32['zdepth'].astype(np.float64) - t.reshape(H, W))[sel].max()
    print('N = %d: %d faces, %d pixels, zdepth error %.3g = %.2f of h^2 / r' % (N, len(f), sel.sum(), err, err / (h * h / RADIUS)))
    assert err <= h * h / RADIUS
    assert np.abs(r32['depth'].astype(np.float64) - (t * calib).reshape(H, W))[sel].max() <= h * h / RADIUS


@pytest.mark.parametrize('N', SPHERES)
def test_float32_against_float64(N):
    _, _, _, _, _, _, r32, r64 = _sphere(N)
    assert np.array_equal(r32['mask'], r64['mask']) and np.array_equal(r32['face'], r64['face'])
    m = r32['mask'] == 1
    assert 300 < m.sum() < m.size - 300
    dd = np.abs(r32['depth'].astype(np.float64) - r64['depth'])[m].max()
    dn = np.abs(r32['normal'].astype(np.float64) - r64['normal']).max()
    db = np.abs(r32['bary'].astype(np.float64) - r64['bary']).max()
    print('N = %d: float32 vs float64: depth %.3g, normal %.3g, bary %.3g' % (N, dd, dn, db))
    assert dd <= 4 * 5.3e-6
    assert dn <= 1e-4                       # a normalised cross product of edges of length h: 2^-24 * (a few) / h relative
    assert (r32['depth'][~m] == np.float32(1e11)).all() and (r32['normal'][~m] == 0).all()
    assert np.abs(np.linalg.norm(r32['normal'][m].astype(np.float64), axis=1) - 1).max() < 1e-6


def _enclosed_invalid(mask):
    """Invalid pixels that cannot be reached from the image border through invalid pixels (4-connected)."""
    inv = mask == 0
    reach = np.zeros_like(inv)
    reach[0], reach[-1], reach[:, 0], reach[:, -1] = inv[0], inv[-1], inv[:, 0], inv[:, -1]
    while True:
        grow = reach.copy()
        grow[1:] |= reach[:-1]
        grow[:-1] |= reach[1:]
        grow[:, 1:] |= reach[:, :-1]
        grow[:, :-1] |= reach[:, 1:]
        grow &= inv
        if np.array_equal(grow, reach):
            return int((inv & ~reach).sum())
        reach = grow


@pytest.mark.parametrize('N', SPHERES)
def test_closed_mesh_is_watertight(N):
    _, _, _, _, _, _, r32, r64 = _sphere(N)
    for r in (r32, r64):
        assert (r['nhits'] % 2 == 0).all() and ((r['nhits'] > 0) == (r['mask'] == 1)).all()
        assert _enclosed_invalid(r['mask']) == 0
    assert r32['nhits'].max() >= 2


# a camera at the mesh frame's origin looking along +z, the ray of pixel (2, 1) exactly (0, 0, 1): K^-1 is exact in float32
_KI0 = Q.k_inv(np.array([[4.0, 0, 2], [0, 4.0, 1], [0, 0, 1]]))
_RT0 = np.concatenate([np.eye(3), np.zeros((3, 1))], 1).astype(np.float32)
_I3 = np.eye(3, dtype=np.float32)
QUAD_V = np.array([[-1, -1, 2], [1, -1, 2], [1, 1, 2], [-1, 1, 2], [0, 0, 2]], np.float32)
DIAG_F = np.array([[0, 1, 2], [0, 2, 3]], np.int32)                      # the diagonal 0-2 passes through (0, 0, 2)
FAN_F = np.array([[4, 0, 1], [4, 1, 2], [4, 2, 3], [4, 3, 0]], np.int32)     # the hub 4 is (0, 0, 2)


@pytest.mark.parametrize('name,faces,nhit', [('diagonal', DIAG_F, 2), ('fan', FAN_F, 4)])
def test_constructed_zero_edge_functions_hit_the_lowest_face(name, faces, nhit):
    H, W, pix = 3, 5, 1 * 5 + 2
    o, e, _, _ = Q.camera(_KI0, _I3, _RT0, H, W)
    assert [float(x[pix]) for x in e] == [0.0, 0.0, 1.0] and [float(x) for x in o] == [0.0, 0.0, 0.0]
    zeros = 0
    for k in range(len(faces)):
        uvw = Q.edge_functions(QUAD_V, faces, _KI0, _I3, _RT0, H, W, pix, k)
        assert not (min(uvw) < 0 < max(uvw))
        zeros += sum(1 for x in uvw if x == 0)
    assert zeros == (2 if name == 'diagonal' else 8)                     # the diagonal once per face, two spokes per fan face
    for r in (Q.render(QUAD_V, faces, _KI0, _I3, _RT0, H, W), Q.render64(QUAD_V, faces, _KI0, _I3, _RT0, H, W)):
        y, x = divmod(pix, W)
        assert r['mask'][y, x] == 1 and r['face'][y, x] == 0 and r['nhits'][y, x] == nhit
        assert abs(r['zdepth'][y, x] - 2) <= (0 if r['zdepth'].dtype == np.float32 else 1e-11)       # float64: d = (0, 0, 1 / (1 + 1e-12))
        assert list(r['normal'][y, x]) == [0, 0, -1]                     # 'image' frame with R = M = 1: towards the camera, x negated
        assert r['mask'].all()                                           # the quad covers the whole 5 x 3 image


def test_triangle_behind_the_camera_is_not_hit():
    back = QUAD_V * np.float32([1, 1, -1])
    for faces in (DIAG_F, FAN_F):
        r = Q.render(back, faces, _KI0, _I3, _RT0, 3, 5)
        assert not r['mask'].any() and (r['face'] == -1).all() and (r['depth'] == np.float32(1e11)).all() and (r['nhits'] == 0).all()


@pytest.mark.parametrize('inward', [False, True])
def test_camera_inside_a_box_hits_on_every_ray(inward):
    v, f = S.box(inward=inward)
    H, W = 9, 11
    Ki = Q.k_inv(Q.intrinsic(H, W, f=3.0))                               # a wide view: all six sides
    RT = Q.look_at(Q.M_DEFAULT.astype(np.float64) @ np.array([0.1, -0.2, 0.15]), Q.M_DEFAULT.astype(np.float64) @ np.array([0.5, 0.4, 0.3]), roll_deg=10)
    r = Q.render(v, f, Ki, Q.M_DEFAULT, RT, H, W, normal_frame='world')
    assert r['mask'].all() and (r['nhits'] == 1).sum() > 0.8 * H * W and len(np.unique(r['face'])) >= 6
    _, e, _, _ = Q.camera64(Ki, Q.M_DEFAULT, RT, H, W)
    n_mesh = r['normal'].reshape(-1, 3).astype(np.float64) @ Q.M_DEFAULT.astype(np.float64)      # M^T (M n)
    assert ((n_mesh * e).sum(1) < 0).all()
    assert np.array_equal(np.abs(n_mesh).max(1), np.ones(H * W))         # axis-aligned sides: exact unit normals
    out = Q.render(*S.box(inward=not inward), Ki, Q.M_DEFAULT, RT, H, W, normal_frame='world')
    for k in ('depth', 'zdepth', 'mask', 'normal'):
        assert r[k].tobytes() == out[k].tobytes()


def test_skip_rules():
    v, f = S.box()
    v2 = np.concatenate([v, [[0.25, 0.25, 0.25], [0.375, 0.375, 0.375], [1, 1, 1], [np.nan, 0, 0]]]).astype(np.float32)
    extra = np.array([[3, 3, 6], [8, 9, 10], [0, 1, 12], [0, -1, 2], [4, 11, 5]], np.int32)   # duplicate vertex, collinear, out of range, NaN
    H, W = 12, 10
    Ki = Q.k_inv(Q.intrinsic(H, W))
    RT = Q.look_at(Q.M_DEFAULT.astype(np.float64) @ np.array([1.2, -1.5, 0.9]))
    plain = Q.render(v, f, Ki, Q.M_DEFAULT, RT, H, W)
    more = Q.render(v2, np.concatenate([extra[:2], f, extra[2:]]), Ki, Q.M_DEFAULT, RT, H, W)
    assert 20 < plain['mask'].sum() < H * W - 20
    for k in ('depth', 'zdepth', 'mask', 'normal', 'bary', 'nhits'):
        assert plain[k].tobytes() == more[k].tobytes()
    assert np.array_equal(more['face'], np.where(plain['face'] >= 0, plain['face'] + 2, -1))
    none = Q.render(v2, extra, Ki, Q.M_DEFAULT, RT, H, W)
    assert not none['mask'].any() and (none['face'] == -1).all()
    bad = RT.copy()
    bad[1, 3] = np.inf
    for r in (Q.render(v, f, Ki, Q.M_DEFAULT, bad, H, W), Q.render64(v, f, Ki, Q.M_DEFAULT, bad, H, W)):
        assert not r['mask'].any() and (r['depth'] == 1e11).all() and (r['normal'] == 0).all()
