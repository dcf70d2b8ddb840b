"""Shape evaluation on the GPU (include/distr_mesh.h, distr/mesh.py, core/evaluation/): marching cubes against its numpy float32
restatement (tests/mesh_restatement.py, same table read from the C++ source), topology and geometry independent of the table, surface
sampling, chamfer distances against float64 brute force (and scipy's KD-tree when it is installed), and the reference's Evaluator
flow end to end with the fixture decoder."""
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
    if name in CLOSED:
        assert (counts == 2).all(), (name, np.bincount(counts))       # closed 2-manifold
    elif name == 'random':
        assert (counts % 2 == 0).all()                                # closed (a few edges where two cells' fans meet: 4 faces)
    else:
        assert (counts == 1).any() and (counts <= 2).all()            # open: boundary edges on the grid faces
    assert f.min() >= 0 and f.max() < len(v) and len(np.unique(f)) == len(v)    # every vertex is used, none twice over an edge


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
    assert np.abs(d - d12 ** 2).max() <= 1e-5 * max(1.0, float((d12 ** 2).max()))


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
