"""Shape evaluation on the GPU (include/distr_mesh.h, distr/mesh.py, core/evaluation/): marching cubes against its numpy float32
restatement (tests/mesh_restatement.py, same table read from the C++ source), topology, orientation and geometry independent of the
table (all 256 cube codes), surface sampling and nearest distances bit for bit against their numpy restatements at the sizes where
the multi-block scans, the second round of the top scan, the grid-stride loop and the chunking of B engage, the float64 distance
sums against math.fsum, chamfer distances against float64 brute force (and scipy's KD-tree when it is installed), and the
reference's Evaluator flow end to end with the fixture decoder."""
import functools
import math
import os

import numpy as np
import pytest

from conftest import GOLDEN
import mesh_restatement as R

pytestmark = pytest.mark.gpu


def _mc(grid, **kw):
    import torch
    from distr import mesh
    v, f = mesh.marching_cubes(torch.from_numpy(np.ascontiguousarray(grid)).cuda(), **kw)
    return v.cpu().numpy(), f.cpu().numpy()


def _random_grid():
    g = np.random.RandomState(3).randn(24, 24, 24).astype(np.float32)
    for ax in range(3):                         # border forced positive: the level set is closed
        idx = [slice(None)] * 3
        idx[ax] = [0, -1]
        g[tuple(idx)] = 1.0
    return g


def _g14(t):
    return np.load(os.path.join(GOLDEN, 'g14_create_mesh_speedup.npz'))['speedup_N64_t%d' % t]


GRIDS = {
    'sphere': lambda: R.sphere_grid(48, (0.11, -0.07, 0.05), 0.6),
    'torus': lambda: R.torus_grid(48, (0.05, 0.03, -0.09), 0.5, 0.2),
    'random': _random_grid,
    'noncubic': lambda: R.sphere_grid(0, (0.02, 0.1, -0.05), 0.55, shape=(21, 34, 27)),
    'g14_t0': lambda: _g14(0),
    'g14_t1': lambda: _g14(1),
    'open': lambda: (lambda a: (a[:, None, None] + 0.3 * a[None, :, None] - 0.2 * a[None, None, :] ** 2 - 0.13).astype(np.float32))(
        np.linspace(-1, 1, 30).astype(np.float32)),
}
CLOSED = ('sphere', 'torus', 'noncubic', 'g14_t0', 'g14_t1')


@pytest.mark.parametrize('name', sorted(GRIDS))
def test_marching_cubes_equals_restatement(name):
    g = GRIDS[name]()
    kw = {}
    if name == 'noncubic':
        kw = dict(origin=(-0.9, -1.1, -1.0), voxel_size=(0.09, 2.0 / 33, 0.075))
    v, f = _mc(g, **kw)
    rv, rf = R.marching_cubes(g, **kw)
    assert len(f) > 100
    assert v.shape == rv.shape and np.array_equal(v.view(np.uint32), rv.view(np.uint32)), name
    assert f.shape == rf.shape and np.array_equal(f, rf), name
    counts = R.edge_use_counts(f)
    fwd, bwd = R.directed_edge_counts(f)
    if name in CLOSED:
        assert (counts == 2).all(), (name, np.bincount(counts))       # closed 2-manifold
        assert (fwd == 1).all() and (bwd == 1).all(), name             # ... consistently oriented: every edge once in each direction
    elif name == 'random':
        assert (counts % 2 == 0).all()                                # closed (a few edges where two cells' fans meet: 4 faces)
        assert np.array_equal(fwd, bwd)                               # ... and as often in one direction as in the other
    else:
        assert (counts == 1).any() and (counts <= 2).all()            # open: boundary edges on the grid faces
    assert f.min() >= 0 and f.max() < len(v) and len(np.unique(f)) == len(v)    # every vertex is used, none twice over an edge


def test_marching_cubes_large_random_grid():
    """106^3 = 1 191 016 points: 582 blocks of MTILE = 2048, so k_mesh_top_scan takes three rounds of 256 block totals (carry twice),
    and more active points than the 4096 x 256 threads k_mc_faces is launched with (distr_mc_emit caps the grid at 4096 blocks), so its
    grid-stride loop runs a second time. No edge_use_counts here: np.unique over 11 M edges takes too long."""
    g = np.random.RandomState(1).randn(106, 106, 106).astype(np.float32)
    active = R.active_points(g)                                         # 1 173 529
    assert g.size > 2 * 256 * 2048 and active > 4096 * 256, active      # the preconditions of the two paths
    rv, rf = R.marching_cubes(g)
    v, f = _mc(g)
    assert v.shape == rv.shape and np.array_equal(v.view(np.uint32), rv.view(np.uint32))
    assert f.shape == rf.shape and np.array_equal(f, rf)


def _awkward_grid(level):
    g = np.random.RandomState(8).randn(12, 10, 9).astype(np.float32)
    g[3:6, 2:5, 2:5] = level                    # a block exactly on the level: t = 0 or 1, coincident vertices
    g[7, 1:4, 6] = -0.0
    g[8, 5, 1:4] = -0.0
    tiny = np.array([1e-39, -1e-39, 3e-41, -2e-42, 1e-44, -1e-45, 7e-40, -4e-43], np.float32)
    assert (tiny != 0).all() and (np.abs(tiny) < np.finfo(np.float32).tiny).all()
    g[1, 6:8, 2:6] = tiny.reshape(2, 4)
    g[10, 2:4, 2:6] = -tiny.reshape(2, 4)
    g[2, 8, 3] = g[9, 7, 7] = np.nan
    g[5, 7, 6] = np.inf
    g[8, 2, 2] = -np.inf
    return g


@pytest.mark.parametrize('level', [0.0, 0.25])
def test_marching_cubes_awkward_values(level):
    g = _awkward_grid(np.float32(level))
    v, f = _mc(g, level=level)
    rv, rf = R.marching_cubes(g, level=level)
    assert len(f) > 100 and f.shape == rf.shape and np.array_equal(f, rf)
    fin = np.isfinite(rv)
    assert v.shape == rv.shape and not fin.all() and np.array_equal(np.isfinite(v), fin)
    assert np.array_equal(v.view(np.uint32)[fin], rv.view(np.uint32)[fin])
    assert f.min() >= 0 and f.max() < len(v)


THIN = {
    '2x2x2': ((2, 2, 2), {}),
    '2x9x7': ((2, 9, 7), {}),
    '9x2x7': ((9, 2, 7), {}),
    '9x7x2': ((9, 7, 2), {}),
    '5x31x2': ((5, 31, 2), dict(origin=(0.5, -2.0, 3.0), voxel_size=(0.3, 0.05, 1.7))),
}


@pytest.mark.parametrize('name', sorted(THIN))
def test_marching_cubes_thin_grids(name):
    shape, kw = THIN[name]
    g = np.random.RandomState(17).randn(*shape).astype(np.float32)
    v, f = _mc(g, **kw)
    rv, rf = R.marching_cubes(g, **kw)
    assert len(f) > 0
    assert v.shape == rv.shape and np.array_equal(v.view(np.uint32), rv.view(np.uint32)), name
    assert f.shape == rf.shape and np.array_equal(f, rf), name


def test_marching_cubes_all_256_cube_codes_closed_and_oriented():
    """Independent of the table: the eight corners of the middle cell of a 4 x 4 x 4 grid of +1 set to -1 where the code has the bit.
    The border is positive, so the level set is closed: every edge in two triangles, once in each direction; normals point towards
    increasing values, so the signed volume is the enclosed inside volume, > 0; one vertex per sign-changing grid edge. Code 0 has no
    inside: no vertex, no triangle, volume 0."""
    for code in range(256):
        g = np.ones((4, 4, 4), np.float32)
        for q, (cx, cy, cz) in enumerate(R.CORNERS):
            if (code >> q) & 1:
                g[1 + cx, 1 + cy, 1 + cz] = -1.0
        ins = g < 0
        crossings = int((ins[:-1] != ins[1:]).sum() + (ins[:, :-1] != ins[:, 1:]).sum() + (ins[:, :, :-1] != ins[:, :, 1:]).sum())
        v, f = _mc(g)
        assert len(v) == crossings, (code, len(v), crossings)
        if code == 0:
            assert len(f) == 0
            continue
        assert len(f) > 0 and f.min() >= 0 and f.max() < len(v), code
        fwd, bwd = R.directed_edge_counts(f)
        assert (fwd == 1).all() and (bwd == 1).all(), (code, np.bincount(fwd), np.bincount(bwd))
        assert R.signed_volume_area(v, f)[0] > 0, code


def test_marching_cubes_topology_and_geometry():
    r = 0.6
    v, f = _mc(R.sphere_grid(48, (0.11, -0.07, 0.05), r))
    assert R.euler(v, f) == 2
    vol, area = R.signed_volume_area(v, f)
    assert abs(vol / (4.0 / 3.0 * np.pi * r ** 3) - 1) < 0.01 and abs(area / (4 * np.pi * r * r) - 1) < 0.01, (vol, area)
    v, f = _mc(R.torus_grid(48, (0.05, 0.03, -0.09), 0.5, 0.2))
    assert R.euler(v, f) == 0 and R.signed_volume_area(v, f)[0] > 0
    # vertices lie on the level set wherever the grid is linear along the edge: level 0.25 of a linear ramp
    ax = np.linspace(-1, 1, 17).astype(np.float32)
    ramp = (ax[:, None, None] + 0 * ax[None, :, None] + 0 * ax[None, None, :]).astype(np.float32)
    v, f = _mc(ramp, level=0.25)
    assert np.abs(v[:, 0] - 0.25).max() < 1e-6


def test_vertices_on_the_fixture_decoders_surface(fixture_decoder):
    import torch
    from core.evaluation import create_sdf_grid
    from core.utils.decoder_utils import decode_sdf
    from distr import mesh
    dec, lat = _decoder(fixture_decoder)
    N = 64
    vs = 2.0 / (N - 1)
    v, f = mesh.marching_cubes(create_sdf_grid(dec, lat, N), 0.0, voxel_size=vs)
    assert len(f) > 1000
    sdf = decode_sdf(dec, lat, v, no_grad=True).reshape(-1)
    assert float(sdf.abs().max()) <= vs, float(sdf.abs().max())
    assert (R.edge_use_counts(f.cpu().numpy()) == 2).all()


def test_determinism_empty_and_refused(tmp_path, monkeypatch, fixture_decoder):
    import torch
    from distr import binding, mesh
    g = _g14(0)
    a, b = _mc(g), _mc(g)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    v, f = _mc(np.ones((9, 10, 11), np.float32))
    assert v.shape == (0, 3) and f.shape == (0, 3)
    for shape in ((1, 5, 5), (5, 1, 5), (5, 5, 1)):
        with pytest.raises(binding.DistrError, match='at least 2'):
            mesh.marching_cubes(torch.ones(shape, device='cuda'))
    # create_mesh on a grid without a crossing: False and no file (the reference's answer when scikit-image raises)
    import sys
    import core.evaluation  # noqa: F401
    cm = sys.modules['core.evaluation.create_mesh']
    dec, lat = _decoder(fixture_decoder)
    monkeypatch.setattr(cm, 'create_sdf_grid', lambda *a, **k: torch.full((16, 16, 16), 0.1, device='cuda'))
    assert cm.create_mesh(dec, lat, str(tmp_path / 'none'), N=16) is False
    assert not os.path.exists(str(tmp_path / 'none.ply'))
    monkeypatch.undo()
    assert cm.create_mesh(dec, lat, str(tmp_path / 'shape'), N=32) is True
    verts, faces = mesh.read_ply(str(tmp_path / 'shape.ply'))
    gv, gf = _mc(cm.create_sdf_grid(dec, lat, 32).cpu().numpy(), voxel_size=2.0 / 31)
    assert np.array_equal(verts, gv) and np.array_equal(faces, gf)


def _tri_coords(v, f, fi, p):
    a, b, c = (v[f[fi, k]].astype(np.float64) for k in range(3))
    e1, e2, d = b - a, c - a, p.astype(np.float64) - a
    n = np.cross(e1, e2)
    plane = np.abs(np.einsum('ij,ij->i', d, n)) / np.linalg.norm(n, axis=1)
    d11, d12, d22 = (e1 * e1).sum(1), (e1 * e2).sum(1), (e2 * e2).sum(1)
    d1, d2 = (d * e1).sum(1), (d * e2).sum(1)
    den = d11 * d22 - d12 * d12
    u = (d22 * d1 - d12 * d2) / den
    w = (d11 * d2 - d12 * d1) / den
    return plane, np.stack([1 - u - w, u, w], 1)


def test_sample_surface():
    import torch
    from distr import mesh
    v, f = mesh.marching_cubes(torch.from_numpy(R.sphere_grid(10, (0.05, 0, -0.03), 0.7)).cuda())
    n = 400000
    p, fi = mesh.sample_surface(v, f, n, seed=5)
    assert p.shape == (n, 3) and fi.shape == (n,) and fi.dtype == torch.int64
    vn, fn, pn, fin = v.cpu().numpy(), f.cpu().numpy(), p.cpu().numpy(), fi.cpu().numpy()
    plane, bary = _tri_coords(vn, fn, fin, pn)
    assert plane.max() < 1e-5 and bary.min() >= -1e-5
    # face hits against the area weights (chi-square, F - 1 degrees of freedom, ~6 sigma)
    areas = 0.5 * np.linalg.norm(np.cross(vn[fn[:, 1]].astype(np.float64) - vn[fn[:, 0]], vn[fn[:, 2]].astype(np.float64) - vn[fn[:, 0]]), axis=1)
    exp = n * areas / areas.sum()
    obs = np.bincount(fin, minlength=len(fn))
    assert (obs[areas == 0] == 0).all()
    k = exp > 0
    chi2, dof = (((obs - exp) ** 2)[k] / exp[k]).sum(), int(k.sum()) - 1
    assert chi2 < dof + 6 * np.sqrt(2 * dof), (chi2, dof)
    # trimesh's folded parallelogram: uniform inside each triangle (mean barycentric coordinates 1/3 on the big faces)
    assert np.abs(bary.mean(0) - 1.0 / 3).max() < 5e-3
    q, qi = mesh.sample_surface(v, f, n, seed=5)
    assert torch.equal(p, q) and torch.equal(fi, qi)
    r, _ = mesh.sample_surface(v, f, n, seed=6)
    assert not torch.equal(p, r)


@functools.lru_cache(maxsize=None)
def _dyadic_soup():
    """526 341 axis-aligned right triangles (257 blocks of 2048 faces + 5: the block offsets of k_area_scan<true> and the second round of
    k_mesh_top_scan<double>), corners on multiples of 1/256, legs from a few multiples of 1/256: every area is a multiple of 2^-17
    and every partial sum is exact in float64 in any order, so the kernel's cumulative area must equal np.cumsum to the bit. About
    1 % of the faces have area 0 (two corners coincide, or the three are collinear), among them a run across face 2048 and the last
    five. Returns (verts, faces, reference points, reference faces of 100 000 samples, areas)."""
    rs = np.random.RandomState(21)
    nf = 526341
    legs = np.array([1, 2, 3, 5, 8, 13, 21, 34])
    la, lb = legs[rs.randint(0, 8, nf)], legs[rs.randint(0, 8, nf)]
    org = rs.randint(-256, 256, (nf, 3))
    ax = rs.randint(0, 3, nf)
    zero = rs.rand(nf) < 0.01
    zero[2040:2057] = True
    zero[-5:] = True
    eye = np.eye(3, dtype=np.int64)
    b = org + la[:, None] * eye[ax]
    c = org + lb[:, None] * eye[(ax + 1) % 3]
    k = np.nonzero(zero)[0]
    b[k[0::2]] = org[k[0::2]]                                    # b == a
    c[k[1::2]] = org[k[1::2]] + 2 * (b[k[1::2]] - org[k[1::2]])  # a, b, c on a line
    verts = (np.stack([org, b, c], 1).reshape(-1, 3) / 256.0).astype(np.float32)
    faces = np.arange(3 * nf, dtype=np.int32).reshape(nf, 3)
    area, _ = R.face_areas(verts, faces)
    assert (area[zero] == 0).all() and (area[~zero] > 0).all()
    assert (area * 2.0 ** 17 == np.round(area * 2.0 ** 17)).all()
    cdf = np.cumsum(area)
    rev = np.cumsum(area[::-1])
    assert cdf[-1] == rev[-1] == math.fsum(area) and np.array_equal(cdf[-1] - cdf[:-1], rev[::-1][1:])
    rp, rf, _ = R.sample_surface(verts, faces, 100000, 31)
    assert (area[rf] > 0).all()
    return verts, faces, rp, rf, area


@pytest.mark.parametrize('n', [1, 255, 256, 257, 100000])
def test_sample_surface_equals_restatement_on_exact_areas(n):
    import torch
    from distr import mesh
    verts, faces, rp, rf, area = _dyadic_soup()
    p, fi = mesh.sample_surface(torch.from_numpy(verts).cuda(), torch.from_numpy(faces).cuda(), n, seed=31)
    p, fi = p.cpu().numpy(), fi.cpu().numpy()
    assert p.shape == (n, 3) and fi.shape == (n,)
    assert np.array_equal(fi, rf[:n]), int((fi != rf[:n]).sum())                 # every sample, no exclusions
    assert np.array_equal(p.view(np.uint32), rp[:n].view(np.uint32))
    assert (area[fi] > 0).all()


def _soup_2049():
    rs = np.random.RandomState(23)
    nv = 700
    v = rs.randn(nv, 3).astype(np.float32)
    f = rs.randint(0, nv, (2049, 3)).astype(np.int32)               # one face more than a block of 2048
    f[5] = (nv, 1, 2)
    f[1000] = (3, -1, 4)
    f[2048] = (1, 2, nv)
    return v, f, (5, 1000, 2048)


@pytest.mark.parametrize('name', ['mc_sphere', 'soup_2049'])
def test_sample_surface_equals_restatement_on_general_meshes(name):
    """Areas that do not sum exactly: the kernel's cumulative area (blocked scan) may differ from np.cumsum by at most nf * 2^-52 of
    the total, so a sample whose pick is closer than that to a boundary between two faces could land on either side and is left out of
    the comparison. The cap is zero such samples (chance per sample 2 * nf^2 * 2^-52, about 2e-9 at 2049 faces): asserted on the
    reference alone, before the GPU's samples are looked at. Seeds 5 and 7 needed no replacement."""
    import torch
    from distr import mesh
    n = 100000
    if name == 'mc_sphere':
        vt, ft = mesh.marching_cubes(torch.from_numpy(R.sphere_grid(10, (0.05, 0, -0.03), 0.7)).cuda())
        v, f, bad, seed = vt.cpu().numpy(), ft.cpu().numpy(), (), 5
        assert len(f) > 100
    else:
        v, f, bad = _soup_2049()
        vt, ft, seed = torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda(), 7
    rp, rf, band = R.sample_surface(v, f, n, seed)
    assert int((band <= len(f) * 2.0 ** -52).sum()) == 0
    area, ok = R.face_areas(v, f)
    assert not ok[list(bad)].any() and (area[list(bad)] == 0).all()
    p, fi = mesh.sample_surface(vt, ft, n, seed=seed)
    p, fi = p.cpu().numpy(), fi.cpu().numpy()
    assert np.array_equal(fi, rf), int((fi != rf).sum())
    assert np.array_equal(p.view(np.uint32), rp.view(np.uint32))
    assert np.isfinite(p).all() and not np.isin(fi, bad).any() and (area[fi] > 0).all()


def _nn_inputs(na, nb, seed):
    """A and B for the nearest-distance tests, by index modulo 8: a unit-sphere cloud; a cluster offset by 4096 in every coordinate
    (float32 differences of such coordinates keep few bits); points within 1e-19 ... 1e-23 of the origin, whose squared distances to
    one another are subnormal or zero; and points of A that are exact copies of points of B. Returns (A, B, indices of the copies)."""
    rs = np.random.RandomState(seed)

    def cloud(n):
        x = rs.randn(n, 3)
        x /= np.linalg.norm(x, axis=1, keepdims=True)
        x = (x + 0.01 * rs.randn(n, 3)).astype(np.float32)
        k = np.arange(n)
        far = k % 8 == 1
        x[far] = (4096.0 + 0.01 * rs.randn(int(far.sum()), 3)).astype(np.float32)
        tiny = k % 8 == 2
        x[tiny] = (rs.randint(-9, 10, (int(tiny.sum()), 3)) * 10.0 ** rs.randint(-23, -19, (int(tiny.sum()), 1))).astype(np.float32)
        return x
    A, B = cloud(na), cloud(nb)
    dup = np.nonzero(np.arange(na) % 8 == 3)[0]
    A[dup] = B[(dup * 7) % nb]
    return A, B, dup


# (na, nb): the launch shape from distr_nearest_sqdist (csrc/distr_api.hip) with MB = NN_TILE = 256: ablocks = ceil(na / 256),
# tiles = ceil(nb / 256), split = min(tiles, ceil(2048 / ablocks), 1024), chunk = ceil(tiles / split) tiles, grid.y = ceil(nb / chunk)
NN_CASES = [
    (1, 1),              # one point each: the partial-tile loop with one entry
    (1, 257),            # tiles 2, split 2, chunks of one tile: a full tile and a tile of one point
    (255, 256),          # one block of A with an idle thread, exactly one full tile
    (256, 255),          # a full block of A, one partial tile
    (257, 513),          # 2 blocks of A (the second with one point), tiles 3, split 3: two full tiles and a tile of one point
    (20000, 7000),       # ablocks 79, tiles 28, split min(28, 26, 1024) = 26, chunk 2 tiles = 512 (t0 advances inside a chunk),
                         # grid.y 14, the last chunk 7000 - 13 * 512 = 344 = one full tile + 88 points
    (300, 300000),       # ablocks 2, tiles 1172, split min(1172, 1024, 1024) = 1024: the cap; chunk 2 tiles, grid.y 586
]


@pytest.mark.parametrize('na,nb', NN_CASES)
def test_nearest_sq_dist_equals_restatement(na, nb):
    """((dx*dx + dy*dy) + dz*dz) in float32 under a min does not depend on the order of B: bit for bit, the chunks' atomic min included."""
    import torch
    from distr import mesh
    A, B, dup = _nn_inputs(na, nb, 100 + na % 97)
    want = R.nearest_sq_dist_f32(A, B)
    assert (want[dup] == 0.0).all()
    if na >= 256:
        sub = want[(want > 0) & (want < np.finfo(np.float32).tiny)]
        assert len(sub) > 0 and (want[np.arange(na) % 8 == 1] < 1.0).all()      # the inputs do what the docstring says
    got = mesh.nearest_sq_dist(torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda())
    assert got.dtype == torch.float32 and got.shape == (na,)
    got = got.cpu().numpy()
    assert (got[dup] == 0.0).all()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), int((got.view(np.uint32) != want.view(np.uint32)).sum())


def test_distance_sums_in_float64_across_scan_rounds():
    """na = 526 341 = 257 blocks of 2048 + 5, so 258 block totals: k_mesh_top_scan<D2> takes a second round of 256 with its carry. The
    sums of d2 and sqrt(d2) against math.fsum (exact) of the GPU's own d2: any order of summing n non-negative float64 terms stays
    within (n - 1) * 2^-53 of the exact sum, relatively."""
    import torch
    from distr import mesh
    na, nb = 526341, 300
    A, B, _ = _nn_inputs(na, nb, 77)
    At, Bt = torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda()
    assert (na + 2047) // 2048 > 256

    def check(x, y, n):
        d2, sums = mesh._nearest(x, y, sums=True)
        d2, sums = d2.cpu().numpy().astype(np.float64), sums.cpu().numpy()
        assert d2.shape == (n,) and sums.dtype == np.float64 and (d2 >= 0).all()
        want = (math.fsum(d2), math.fsum(np.sqrt(d2)))
        print('n %d: sums %r, fsum %r' % (n, tuple(sums), want))
        for k in range(2):
            assert want[k] > 0 and abs(sums[k] - want[k]) <= n * 2.0 ** -53 * want[k], (k, sums[k], want[k])
        return sums
    s12, s21 = check(At, Bt, na), check(Bt, At, nb)
    d21, d12 = mesh.chamfer(At, Bt, separate=True)
    assert d12 == np.float64(s12[0] / na) and d21 == np.float64(s21[0] / nb)
    # no point in A: both sums are 0, nothing is read
    d2, sums = mesh._nearest(At[:0], Bt, sums=True)
    assert d2.shape == (0,) and tuple(sums.cpu().numpy()) == (0.0, 0.0)


def _chamfer_f64(p1, p2):
    import torch
    a, b = torch.from_numpy(p1).double(), torch.from_numpy(p2).double()

    def nn(x, y):
        return torch.cat([torch.cdist(x[i:i + 500], y).min(1).values for i in range(0, len(x), 500)])
    d12, d21 = nn(a, b), nn(b, a)                 # over p1, over p2
    return d12.numpy(), d21.numpy()


def test_chamfer_against_float64_brute_force():
    from core.evaluation import compute_chamfer_distance, compute_chamfer_distance_separate
    from distr import mesh
    import torch
    rs = np.random.RandomState(11)
    p1 = rs.randn(3000, 3).astype(np.float32)
    p1 /= np.linalg.norm(p1, axis=1, keepdims=True)
    p2 = (rs.randn(2000, 3) * 0.6).astype(np.float32)
    d12, d21 = _chamfer_f64(p1, p2)
    sq = np.mean(d21 ** 2) + np.mean(d12 ** 2)
    got = compute_chamfer_distance(p1, p2)
    assert isinstance(got, np.float64) and abs(got / sq - 1) <= 1e-5, (got, sq)
    got = compute_chamfer_distance(p1, p2, use_square_dist=False)
    assert abs(got / (np.mean(d21) + np.mean(d12)) - 1) <= 1e-5
    s21, s12 = compute_chamfer_distance_separate(p1, p2)
    assert abs(s21 / np.mean(d21 ** 2) - 1) <= 1e-5 and abs(s12 / np.mean(d12 ** 2) - 1) <= 1e-5
    t = mesh.chamfer(torch.from_numpy(p1).cuda(), torch.from_numpy(p2).cuda(), separate=True)
    assert t == (s21, s12)
    assert compute_chamfer_distance(p1, p1) == 0.0
    d = mesh.nearest_sq_dist(torch.from_numpy(p1).cuda(), torch.from_numpy(p2).cuda()).cpu().numpy()
    assert (np.abs(d - d12 ** 2) <= 6 * 2.0 ** -24 * d12 ** 2).all()      # per point: 5 float32 roundings to first order, the min keeps it


def test_chamfer_against_scipy_kdtree():
    spatial = pytest.importorskip('scipy.spatial')
    from core.evaluation import compute_chamfer_distance
    rs = np.random.RandomState(12)
    p1 = rs.randn(30000, 3).astype(np.float32)
    p1 /= np.linalg.norm(p1, axis=1, keepdims=True)
    p2 = (p1 + 0.01 * rs.randn(30000, 3)).astype(np.float32)
    one, _ = spatial.cKDTree(p1).query(p2)
    two, _ = spatial.cKDTree(p2).query(p1)
    want = np.mean(np.square(one)) + np.mean(np.square(two))
    assert abs(compute_chamfer_distance(p1, p2) / want - 1) <= 1e-5


def _decoder(fixture_decoder):
    import torch
    from core.graph.deep_sdf_decoder import Decoder
    Ws, bs, latent = fixture_decoder
    dec = Decoder(256, [512] * 8, norm_layers=(), latent_in=[4])
    dec.load_state_dict({('lin%d.%s' % (l, n)): torch.from_numpy(a) for l, (W, b) in enumerate(zip(Ws, bs)) for n, a in (('weight', W), ('bias', b))})
    return dec.cuda(), torch.from_numpy(latent).cuda()


def test_evaluator_end_to_end(tmp_path, capsys, fixture_decoder):
    import torch
    import core.evaluation as ce
    from core.evaluation import Evaluator, latent_vec_to_points
    from core.inv_optimizer import optimize_single_view
    from core.sdfrenderer import SDFRenderer
    from distr import fixture, mesh
    assert Evaluator.__module__ == 'core.evaluation.gpu_evaluator'        # no reference checkout on this path
    dec, lat = _decoder(fixture_decoder)
    ev = Evaluator(dec)
    fname = str(tmp_path / 'mesh.ply')
    pts = ev.latent_vec_to_points(lat, N=128, num_points=5000, fname=fname)
    assert isinstance(pts, np.ndarray) and pts.shape == (5000, 3)
    v, f = mesh.read_ply(fname)
    assert len(f) > 1000 and f.max() < len(v)
    other = latent_vec_to_points(dec, lat, N=128, num_points=5000, seed=1)
    for scale in (3.0, 1.5):            # a perturbed code (make_latent: std 0.1) that still has a surface
        pert = latent_vec_to_points(dec, lat + scale * torch.from_numpy(fixture.make_latent(5)).cuda(), N=128, num_points=5000)
        if pert is not None:
            break
    assert pert is not None
    c_seed, c_pert = ev.compute_chamfer_distance(pts, other), ev.compute_chamfer_distance(pts, pert)
    print('chamfer: two seeds %.3e, perturbed latent %.3e' % (c_seed, c_pert))
    assert 0 < c_seed and 4 * c_seed < c_pert
    s = ev.compute_chamfer_distance(pts, pert, separate=True)
    assert abs(s[0] + s[1] - c_pert) <= 1e-12 * c_pert
    assert ce.sample_points_from_ply_file(fname, 100).shape == (100, 3)
    # the optimisation loop with the evaluator every iteration (optimize_single.py:87-98)
    H = W = 48
    K = fixture.make_intrinsic(H, W)
    Rm, T = fixture.make_camera(30, 20, 1.6, 10)
    r = SDFRenderer(dec, K, img_hw=(H, W), march_step=30, buffer_size=3, use_depth2normal=True)
    RT = torch.from_numpy(np.concatenate([Rm, T[:, None]], 1).astype(np.float32)).cuda()
    with torch.no_grad():
        d, n, m, _ = r.render(lat, RT[:, :3], RT[:, 3], no_grad=True)
    gt = {'depth': d, 'normal': n, 'silhouette': m}
    code = (lat + 0.5 * torch.from_numpy(fixture.make_latent(6)).cuda()).detach().requires_grad_(True)
    opt = torch.optim.Adam([code], lr=1e-2)
    wd = dict(w_depth=10.0, w_normal=5.0, w_mask_gt=1.0, w_mask_out=1.0, w_l2reg=1.0)
    capsys.readouterr()
    optimize_single_view([r], ev, opt, code, RT, gt, wd, num_iters=2, points_gt=pts, test_step=1, silent=False, vis_folder=str(tmp_path / 'vis'))
    out = capsys.readouterr().out
    assert out.count('CHAMFER DISTANCE:') == 2, out
    assert os.path.exists(str(tmp_path / 'vis' / 'output_1.ply'))
