"""Signed distances to a triangle mesh and SDF training samples on the GPU (include/distr_mesh.h: distr_mesh_sdf, distr_sdf_queries;
distr/mesh.py: signed_distance, sdf_samples): the squared distance and the nearest face bit for bit against the numpy float32
restatement (tests/mesh_sdf_restatement.py, validated on the CPU by tests/test_mesh_sdf_host.py) at the tile and chunk edges, the
winding number against the float64 restatement within twice the float32 floor, the inside / outside property on marching-cubes
meshes, the skip rules, determinism, the query generator, and the chain mesh -> samples -> one training step end to end."""
import functools

import numpy as np
import pytest

import mesh_restatement as R
import mesh_sdf_restatement as S

pytestmark = pytest.mark.gpu
CH = S.SDF_CHUNK


def _sd(v, f, Q):
    import torch
    from distr import mesh
    out = mesh.signed_distance(torch.from_numpy(np.ascontiguousarray(v)).cuda(), torch.from_numpy(np.ascontiguousarray(f)).cuda(),
                               torch.from_numpy(np.ascontiguousarray(Q)).cuda(), details=True)
    assert out[0].dtype == torch.float32 and out[1].dtype == torch.float32 and out[2].dtype == torch.float32 and out[3].dtype == torch.int64
    assert all(o.shape == (len(Q),) for o in out)
    return tuple(o.cpu().numpy() for o in out)


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _check_d2_face(got, want):
    """squared distance and nearest face bit for bit; the signed distance is the GPU's own sign on the square root of that."""
    sdf, d2, w, face = got
    assert np.array_equal(_bits(d2), _bits(want[1])), int((_bits(d2) != _bits(want[1])).sum())
    assert np.array_equal(face, want[3]), int((face != want[3]).sum())
    with np.errstate(invalid='ignore'):
        assert np.array_equal(_bits(sdf), _bits(np.where(np.abs(w) > np.float32(0.5), np.float32(-1), np.float32(1)) * np.sqrt(d2)))


def _check_winding(name, w, w32, w64):
    """The bar: twice the error of the numpy float32 evaluation of the same formula on the same inputs; and below 0.05 whatever that
    is, so that no sign can flip away from w = 0.5."""
    floor = float(np.abs(w32.astype(np.float64) - w64).max())
    err = float(np.abs(w.astype(np.float64) - w64).max())
    print('%s: winding error GPU %.3g, numpy float32 %.3g (bar %.3g)' % (name, err, floor, 2 * floor))
    assert err < 0.05, (name, err)
    assert err <= 2 * floor, (name, err, floor)


def test_one_triangle_regions_and_zero_distances():
    Q = np.array([c[0] for c in S.TRI_CASES], np.float32)
    got = _sd(S.TRI_V, S.TRI_F, Q)
    want = S.signed_distance(S.TRI_V, S.TRI_F, Q)
    _check_d2_face(got, want)
    exact = ((Q.astype(np.float64) - np.array([c[2] for c in S.TRI_CASES], np.float64)) ** 2).sum(1)
    assert np.array_equal(got[1].astype(np.float64), exact) and (got[1][7:] == 0).all() and (got[3] == 0).all()
    assert (got[0] >= 0).all() and np.abs(got[2]).max() <= 0.5          # one triangle: never more than half the sphere


@functools.lru_cache(maxsize=None)
def _soup(nf, nq):
    """A random triangle soup and queries around it; every 50th face from the 25th repeats a vertex (skipped), query 3 is corner a of
    a counted face (distance exactly 0: p = a), query 4 corner c of another (p = a + ac, which need not round to c), and two faces are
    listed twice (ties)."""
    rs = np.random.RandomState(1000 + nf + 7 * nq)
    nv = max(3, min(400, nf))
    v = rs.randn(nv, 3).astype(np.float32)
    f = rs.randint(0, nv, (nf, 3)).astype(np.int32)
    f[25::50, 1] = f[25::50, 0]
    for k in {0, min(1, nf - 1), min(nf - 1, 200)}:
        f[k] = rs.choice(nv, 3, replace=False)
    if nf > 300:
        f[nf - 1] = f[2]
        f[260] = f[7]
    Q = (rs.randn(nq, 3) * 1.2).astype(np.float32)
    if nq > 4:
        Q[3], Q[4] = v[f[min(1, nf - 1), 0]], v[f[min(nf - 1, 200), 2]]
    return v, f, Q, S.signed_distance(v, f, Q)


SOUPS = [(nf, 257) for nf in (1, 255, 256, 257, CH - 1, CH, CH + 1, 2 * CH + 1)] + [(257, nq) for nq in (1, 255, 256)]


@pytest.mark.parametrize('nf,nq', SOUPS)
def test_random_soups_equal_restatement(nf, nq):
    """One block of queries and two, a full tile of faces and one more or less, a full chunk of CH faces and one more or less, two
    chunks and a face (the atomic min between chunks; the tie of a face listed in two chunks goes to the lower index)."""
    v, f, Q, want = _soup(nf, nq)
    got = _sd(v, f, Q)
    _check_d2_face(got, want)
    assert np.isfinite(got[2]).all()
    if nq > 4:
        assert got[1][3] == 0 and got[1][4] < 1e-12


@functools.lru_cache(maxsize=None)
def _box_case(kind):
    v, f = S.box(inward=(kind == 'inward'))
    if kind == 'open':
        f = f[:-2]                                   # the lid z = +1/2 removed
    Q = (np.random.RandomState(5).rand(2000, 3) * 2 - 1).astype(np.float32)
    return v, f, Q, S.signed_distance(v, f, Q), S.signed_distance(v, f, Q, np.float64)


@functools.lru_cache(maxsize=None)
def _sphere_case():
    g = R.sphere_grid(33, (0.03, -0.02, 0.01), 0.5)
    v, f = R.marching_cubes(g)
    assert v.shape == (1210, 3) and f.shape == (2416, 3) and (R.edge_use_counts(f) == 2).all() and R.euler(v, f) == 2
    ax = np.linspace(-1, 1, 33).astype(np.float32)
    P = np.stack(np.meshgrid(ax, ax, ax, indexing='ij'), -1).reshape(-1, 3)
    sub = np.random.RandomState(6).choice(len(P), 3000, replace=False)
    Q, val = np.ascontiguousarray(P[sub]), g.reshape(-1)[sub]
    assert np.abs(val).min() > 1e-4
    return v, f, Q, val, S.signed_distance(v, f, Q), S.signed_distance(v, f, Q, np.float64)


def test_box_distance_winding_and_closed_form():
    v, f, Q, w32, w64 = _box_case('outward')
    got = _sd(v, f, Q)
    _check_d2_face(got, w32)
    _check_winding('box', got[2], w32[2], w64[2])
    want = S.box_sdf(Q)
    assert np.array_equal(got[0] < 0, want < 0) and np.abs(got[0] - want).max() <= 30 * 2.0 ** -24 * 4     # as the host test's float32 bound


def test_sphere_winding_is_the_grids_sign():
    """At grid points of the marching-cubes sphere: winding > 0.5 exactly where the grid value is negative (the mesh separates the
    grid's negative points from the others whatever the values are), and the winding bar against float64."""
    v, f, Q, val, w32, w64 = _sphere_case()
    assert np.abs(w64[2] - (val < 0)).max() < 1e-12                  # the yardstick itself: 0 or 1
    got = _sd(v, f, Q)
    _check_d2_face(got, w32)
    assert np.array_equal(got[2] > 0.5, val < 0)
    assert np.array_equal(got[0] < 0, val < 0)
    _check_winding('sphere', got[2], w32[2], w64[2])


def test_skipped_faces_change_no_byte():
    v, f, Q, w32, _ = _box_case('outward')
    v2 = np.concatenate([v, [[0.25, 0.25, 0.25], [0.375, 0.375, 0.375], [1, 1, 1], [np.nan, 0, 0]]]).astype(np.float32)
    extra = np.array([[3, 3, 6], [8, 9, 10], [0, 1, 12], [0, -1, 2], [4, 11, 5]], np.int32)   # duplicate vertex, collinear, out of range, NaN
    assert not S.face_records(v2, extra)[3].any()
    a, b = _sd(v, f, Q), _sd(v2, np.concatenate([f, extra]), Q)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    # nothing but skipped faces; queries that are not finite
    Qb = np.array([[0, 0, 0], [np.nan, 0, 0], [0, -np.inf, 0.5], [0.1, 0.2, np.inf]], np.float32)
    sdf, d2, w, face = _sd(v2, extra, Qb)
    assert sdf[0] == np.inf and d2[0] == np.inf and w[0] == 0 and face[0] == -1
    assert np.isnan(sdf[1:]).all() and np.isnan(d2[1:]).all() and np.isnan(w[1:]).all() and list(face[1:]) == [-1, -1, -1]
    sdf, _, _, face = _sd(v2, np.concatenate([f, extra]), Qb)
    assert sdf[0] == -0.5 and 0 <= face[0] < 12 and np.isnan(sdf[1:]).all() and list(face[1:]) == [-1, -1, -1]
    from distr import binding, mesh
    import torch
    with pytest.raises(ValueError, match='no triangles'):
        mesh.signed_distance(torch.from_numpy(v).cuda(), torch.zeros((0, 3), dtype=torch.int32, device='cuda'), torch.from_numpy(Q).cuda())
    ctx = mesh._context(torch.device('cuda', 0))
    vt, qt, out = torch.from_numpy(v).cuda(), torch.from_numpy(Q).cuda(), torch.empty(len(Q), device='cuda')
    rc = ctx.L.distr_mesh_sdf(ctx.h, binding.ptr(vt), len(v), binding.ptr(vt), 0, binding.ptr(qt), len(Q), binding.ptr(out), None, None, None,
                              binding.ptr(out), 4, None)
    assert rc == -1                                                  # DISTR_ERR_INVALID_ARG: no faces
    assert mesh.signed_distance(vt, torch.from_numpy(f).cuda(), qt[:0]).shape == (0,)


def test_open_box_fractional_winding():
    v, f, Q, w32, w64 = _box_case('open')
    got = _sd(v, f, Q)
    _check_d2_face(got, w32)
    _check_winding('open box', got[2], w32[2], w64[2])
    frac = (np.abs(w64[2]) > 0.01) & (np.abs(w64[2]) < 0.99)
    assert frac.sum() > 500                                            # an open mesh: fractional winding numbers
    clear = np.abs(np.abs(w64[2]) - 0.5) > 0.05
    assert clear.sum() > 1000 and np.array_equal((got[0] < 0)[clear], (np.abs(w64[2]) > 0.5)[clear])


def test_inward_wound_box_gives_the_same_bytes():
    v, f, Q, w32, _ = _box_case('outward')
    vi, fi, Qi, wi32, wi64 = _box_case('inward')
    a, b = _sd(v, f, Q), _sd(vi, fi, Qi)
    assert a[0].tobytes() == b[0].tobytes()
    inside = S.box_sdf(Q) < 0
    assert (b[2][inside] < -0.5).all() and (np.abs(b[2][~inside]) < 0.5).all() and (a[2][inside] > 0.5).all()
    _check_winding('inward box', b[2], wi32[2], wi64[2])


def test_determinism_prefix_and_pieces(monkeypatch):
    from distr import mesh
    v, f, Q, _, w32, _ = _sphere_case()
    a, b = _sd(v, f, Q), _sd(v, f, Q)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    head = _sd(v, f, Q[:257])
    for x, y in zip(a, head):
        assert x[:257].tobytes() == y.tobytes()
    # pieces of 256 queries (the workspace bound) instead of one call: the same bytes
    monkeypatch.setattr(mesh, '_SDF_WS_BYTES', 1)
    c = _sd(v, f, Q)
    for x, y in zip(a, c):
        assert x.tobytes() == y.tobytes()


def test_sdf_samples_queries_split_and_npz(tmp_path):
    import torch
    from distr import mesh
    v, f = _sphere_case()[:2]
    vt, ft = torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda()
    ns, nu, seed, h = 1000, 300, 3, 0.75
    sig = (0.005 ** 0.5, 0.0005 ** 0.5)
    pts, _ = mesh.sample_surface(vt, ft, ns, seed=seed)
    q = mesh.sdf_queries(pts, sig, nu, h, seed)
    assert q.shape == (2 * ns + nu, 3) and q.dtype == torch.float32
    qn, pn = q.cpu().numpy(), pts.cpu().numpy()
    q32, q64 = S.sdf_queries(pn, sig[0], sig[1], nu, h, seed), S.sdf_queries(pn, sig[0], sig[1], nu, h, seed, np.float64)
    assert np.array_equal(_bits(qn[2 * ns:]), _bits(q32[2 * ns:]))                     # the uniforms: bit for bit
    assert (qn[2 * ns:] >= -h).all() and (qn[2 * ns:] < h).all()
    floor = np.abs(q32[:2 * ns].astype(np.float64) - q64[:2 * ns]).max()
    err = np.abs(qn[:2 * ns].astype(np.float64) - q64[:2 * ns]).max()
    print('perturbed surface points: error GPU %.3g, numpy float32 %.3g' % (err, floor))
    assert err <= 2 * floor
    assert np.array_equal(mesh.sdf_queries(pts[:10], sig, 5, h, seed).cpu().numpy(), np.concatenate([qn[:20], qn[2 * ns:2 * ns + 5]]))
    # the samples: the queries with their signed distance, split by sign in query order
    sdf = mesh.signed_distance(vt, ft, q)
    smp = mesh.sdf_samples(vt, ft, ns, seed=seed, n_uniform=nu, half_extent=h)
    pos, neg = smp['pos'], smp['neg']
    assert pos.dtype == torch.float32 and pos.shape[1] == 4 and neg.shape[1] == 4 and len(pos) + len(neg) == 2 * ns + nu
    assert (pos[:, 3] >= 0).all() and (neg[:, 3] < 0).all() and len(pos) > 500 and len(neg) > 500
    rows = torch.cat([q, sdf[:, None]], 1)
    assert torch.equal(pos, rows[sdf >= 0]) and torch.equal(neg, rows[sdf < 0])
    dflt = mesh.sdf_samples(vt, ft, 50, seed=seed)
    assert len(dflt['pos']) + len(dflt['neg']) == 2 * 50 + 5
    # near the surface the signed distance is the sphere's, to the mesh's accuracy: a chord as long as a cell's diagonal (sqrt(3) / 16)
    # sags (sqrt(3) / 16)^2 / (8 * 0.5) = 2.9e-3 below the sphere, and the vertices sit on linearly interpolated grid values that are
    # off by as much again
    x = rows[:2 * ns].cpu().numpy().astype(np.float64)
    true = np.linalg.norm(x[:, :3] - [0.03, -0.02, 0.01], axis=1) - 0.5
    assert np.abs(x[:, 3] - true).max() < 6e-3
    fn = str(tmp_path / 's.npz')
    mesh.write_sdf_npz(fn, smp)
    back = mesh.read_sdf_npz(fn)
    assert np.array_equal(back['pos'], pos.cpu().numpy()) and np.array_equal(back['neg'], neg.cpu().numpy())


def _decoder(fixture_decoder):
    import torch
    from core.graph.deep_sdf_decoder import Decoder
    Ws, bs, latent = fixture_decoder
    dec = Decoder(256, [512] * 8, norm_layers=(), latent_in=[4])
    dec.load_state_dict({('lin%d.%s' % (l, n)): torch.from_numpy(a) for l, (W, b) in enumerate(zip(Ws, bs)) for n, a in (('weight', W), ('bias', b))})
    return dec.cuda().eval(), torch.from_numpy(latent).cuda()


def test_mesh_to_samples_to_training_step(fixture_decoder):
    """decoder -> grid (N = 32) -> marching cubes -> winding at the grid points -> sdf_samples -> decode_sdf_train forward and backward."""
    import torch
    from core.evaluation import create_sdf_grid
    from core.evaluation.create_mesh import get_samples
    from core.utils.decoder_utils import decode_sdf_train
    from distr import mesh
    dec, lat = _decoder(fixture_decoder)
    N = 32
    grid = create_sdf_grid(dec, lat, N)
    v, f = mesh.marching_cubes(grid, 0.0, voxel_size=2.0 / (N - 1))
    assert len(f) > 1000 and (R.edge_use_counts(f.cpu().numpy()) == 2).all()          # the precondition: a closed mesh
    g = grid.reshape(-1)
    assert float(g.abs().min()) > 0
    sdf, d2, w, face = mesh.signed_distance(v, f, get_samples(N, device=v.device), details=True)
    assert torch.equal(w > 0.5, g < 0) and torch.equal(sdf < 0, g < 0)
    assert int((g < 0).sum()) > 1000 and int(face.min()) >= 0 and int(face.max()) < len(f)
    smp = mesh.sdf_samples(v, f, 2000, seed=1)
    rows = torch.cat([smp['pos'], smp['neg']])
    assert rows.shape == (2 * 2000 + 200, 4) and bool(torch.isfinite(rows).all())
    pred = decode_sdf_train(dec, lat.reshape(1, -1), rows[None, :, :3].contiguous(), clamp_dist=0.1)
    loss = (pred.reshape(-1) - rows[:, 3].clamp(-0.1, 0.1)).abs().mean()
    loss.backward()
    assert bool(torch.isfinite(loss)) and float(loss.detach()) > 0
    grads = [p.grad for p in dec.parameters()]
    assert all(gr is not None and bool(torch.isfinite(gr).all()) for gr in grads)
    assert all(float(gr.abs().max()) > 0 for gr in grads)
