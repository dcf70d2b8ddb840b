"""CPU-only checks of the signed-distance feature: the new part of the mesh C ABI against the binding, and the numpy restatements
(tests/mesh_sdf_restatement.py) that tests/test_gpu_mesh_sdf.py compares the kernels with, validated here against independent
statements: the closed-form distance to a cube, constructed queries for each of a triangle's seven regions, the tie and skip rules,
and the statistics of the query generator. Plus the host-side helpers of distr.mesh (unit-sphere normalisation, the npz layout)."""
import os

import numpy as np
import pytest

from conftest import ROOT
import mesh_sdf_restatement as S


def test_sdf_abi_exported_and_chunk_constant():
    from distr import binding, mesh
    for name in ('distr_mesh_sdf_workspace_bytes', 'distr_mesh_sdf', 'distr_sdf_queries'):
        assert name in binding.MESH_EXPORTS
    hdr = open(os.path.join(ROOT, 'include', 'distr_mesh.h')).read()
    assert 'distr_mesh_sdf(' in hdr and 'distr_sdf_queries(' in hdr
    binding.build_library()
    L = binding.lib()
    ws = L.distr_mesh_sdf_workspace_bytes
    assert ws(0, 10) == 0 and ws(10, 0) == 0
    # one float64 row of nq per chunk of SDF_CHUNK faces: the constant of the library is the one Python and the restatement use
    CH = mesh.SDF_CHUNK
    assert CH == S.SDF_CHUNK and CH % S.SDF_TILE == 0
    assert ws(256, 1) == ws(256, CH) and ws(256, CH + 1) - ws(256, CH) == 256 * 8 and ws(256, 2 * CH + 1) - ws(256, 2 * CH) == 256 * 8
    assert ws(256, CH) >= 256 * 16
    # calls without a context are refused, not crashed
    assert L.distr_mesh_sdf(None, None, 0, None, 0, None, 0, None, None, None, None, None, 0, None) == -1
    assert L.distr_sdf_queries(None, None, 0, 0.0, 0.0, 0, 1.0, 0, None, None) == -1


def test_float64_restatement_equals_the_cubes_closed_form():
    """The cube [-1/2, 1/2]^3 has dyadic coordinates, so the face records are exact; what remains is float64 rounding in the closest
    point and the norm: each of about 30 operations on numbers below 4 adds at most 2^-53 * 4, so 1e-14 bounds the distance error. The
    winding number of a closed mesh is exactly 0 or 1; twelve arctan2 values of magnitude <= pi, each good to a few 2^-53 relative
    besides the rounding of its arguments, leave it within 1e-13 unless the point is on the surface (none of these is: the smallest
    distance is asserted)."""
    v, f = S.box()
    rs = np.random.RandomState(0)
    Q = (rs.rand(4000, 3) * 2 - 1).astype(np.float32)
    want = S.box_sdf(Q)
    assert np.abs(want).min() > 1e-5 and (want < 0).sum() > 300
    sdf, d2, w, face = S.signed_distance(v, f, Q, np.float64)
    err = np.abs(sdf - want).max()
    werr = np.abs(w - (want < 0)).max()
    print('box, float64: max |sdf - closed form| %.3g, max |w - {0, 1}| %.3g' % (err, werr))
    assert err <= 1e-14 and werr <= 1e-13
    assert np.array_equal(d2, sdf * sdf) or np.abs(np.sqrt(d2) - np.abs(sdf)).max() == 0
    assert (face >= 0).all() and (face < 12).all()
    # the float32 restatement: the same signs, distances to float32 accuracy (about 30 roundings of 2^-24 on numbers below 4)
    s32, d32, w32, f32 = S.signed_distance(v, f, Q)
    assert s32.dtype == np.float32 and w32.dtype == np.float32 and f32.dtype == np.int32
    assert np.array_equal(s32 < 0, want < 0) and np.abs(s32 - want).max() <= 30 * 2.0 ** -24 * 4
    # the inward-wound cube: winding -1 inside, the same signed distances
    vi, fi = S.box(inward=True)
    si, _, wi, _ = S.signed_distance(vi, fi, Q, np.float64)
    assert np.abs(wi + (want < 0)).max() <= 1e-13 and np.abs(si - want).max() <= 1e-14


TRI_V, TRI_F, TRI_CASES = S.TRI_V, S.TRI_F, S.TRI_CASES


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_seven_regions_of_one_triangle(dtype):
    Q = np.array([c[0] for c in TRI_CASES], np.float32)
    dist2, half, reg = S.pair_terms(TRI_V, TRI_F, Q, dtype)
    assert [S.REGIONS[r] for r in reg[:, 0]] == [c[1] for c in TRI_CASES]
    assert set(reg[:7, 0]) == set(range(7))                                      # each region once among the first seven
    want = ((Q.astype(np.float64) - np.array([c[2] for c in TRI_CASES], np.float64)) ** 2).sum(1)
    assert np.array_equal(dist2[:, 0].astype(np.float64), want)                  # dyadic numbers: exact
    assert (dist2[7:, 0] == 0).all() and (want[:7] > 0).all()
    # listing the corners as (c, a, b) moves the regions' names with them and leaves the distances
    names = {'vertex a': 'vertex b', 'vertex b': 'vertex c', 'vertex c': 'vertex a', 'edge ab': 'edge bc', 'edge ac': 'edge ab',
             'edge bc': 'edge ac', 'interior': 'interior'}
    d2r, _, regr = S.pair_terms(TRI_V, np.roll(TRI_F, 1, 1), Q, dtype)
    assert np.array_equal(d2r, dist2)
    assert [S.REGIONS[r] for r in regr[:7, 0]] == [names[c[1]] for c in TRI_CASES[:7]]
    # the solid angle of the triangle seen from below its interior is positive towards the side its normal leaves ... and flips above
    below, above = np.array([[1, 1, 0.0]], np.float32), np.array([[1, 1, 2.0]], np.float32)
    hb, ha = S.pair_terms(TRI_V, TRI_F, below, dtype)[1][0, 0], S.pair_terms(TRI_V, TRI_F, above, dtype)[1][0, 0]
    assert hb > 0 and ha == -hb


def test_tie_rule_lowest_face_index():
    """Two triangles that share the edge (0, 0, 0) - (0, 0, 4) and a query whose closest point lies on it: equal distances (dyadic, so
    exactly equal), the lower index wins, whichever triangle it is; and a triangle listed twice."""
    v = np.array([[0, 0, 0], [0, 0, 4], [4, 0, 0], [0, 4, 0]], np.float32)
    f = np.array([[0, 1, 2], [1, 0, 3]], np.int32)
    Q = np.array([[-1.0, -1.0, 1.5], [-2.0, -0.5, 3.0]], np.float32)
    for dtype in (np.float32, np.float64):
        d2 = S.pair_terms(v, f, Q, dtype)[0]
        assert np.array_equal(d2[:, 0], d2[:, 1]) and np.array_equal(d2[:, 0].astype(np.float64), [2.0, 4.25])
        assert list(S.signed_distance(v, f, Q, dtype)[3]) == [0, 0]
        assert list(S.signed_distance(v, f[::-1], Q, dtype)[3]) == [0, 0]
        three = np.array([[1, 0, 3], [0, 1, 2], [0, 1, 2]], np.int32)
        assert list(S.signed_distance(v, three, np.array([[2.0, -3.0, 1.0]], np.float32), dtype)[3]) == [1]


def test_skip_rules():
    v, f = S.box()
    nv = len(v)
    v2 = np.concatenate([v, [[np.nan, 0, 0], [0, np.inf, 0], [0.25, 0.25, 0.25], [0.5, 0.5, 0.5], [1, 1, 1]]]).astype(np.float32)
    extra = np.array([[0, 0, 5],            # two corners coincide
                      [nv + 2, nv + 3, nv + 4],   # three corners on a line
                      [0, 1, nv + 5], [-1, 2, 3],  # a vertex outside the array
                      [0, 1, nv], [2, nv + 1, 3]], np.int32)  # a NaN, an infinite vertex
    f2 = np.concatenate([f[:5], extra, f[5:]])
    _, _, _, ok = S.face_records(v2, f2)
    assert list(np.nonzero(~ok)[0]) == [5, 6, 7, 8, 9, 10]
    Q = (np.random.RandomState(1).rand(500, 3) * 2 - 1).astype(np.float32)
    keep = np.concatenate([np.arange(5), np.arange(11, 18)])
    for dtype in (np.float32, np.float64):
        a = S.signed_distance(v, f, Q, dtype)
        b = S.signed_distance(v2, f2, Q, dtype)
        for x, y in zip(a[:3], b[:3]):
            assert x.tobytes() == y.tobytes()
        assert np.array_equal(keep[a[3]], b[3])
        # nothing but skipped faces: +inf, face -1, winding 0; a query that is not finite: NaN, -1
        Qb = np.array([[0, 0, 0], [np.nan, 0, 0], [0, -np.inf, 0.5]], np.float32)
        sdf, d2, w, face = S.signed_distance(v2, extra, Qb, dtype)
        assert sdf[0] == np.inf and d2[0] == np.inf and w[0] == 0 and face[0] == -1
        assert np.isnan(sdf[1:]).all() and np.isnan(d2[1:]).all() and np.isnan(w[1:]).all() and list(face[1:]) == [-1, -1]
        sdf, _, _, face = S.signed_distance(v2, f2, Qb, dtype)
        assert sdf[0] == -0.5 and face[0] >= 0 and np.isnan(sdf[1:]).all() and list(face[1:]) == [-1, -1]


def test_query_generator_restatement():
    ns, nu, seed = 20000, 5000, 7
    rs = np.random.RandomState(2)
    surf = rs.randn(ns, 3).astype(np.float32)
    sa, sb, h = np.float32(np.sqrt(0.005)), np.float32(np.sqrt(0.0005)), np.float32(0.75)
    q = S.sdf_queries(surf, sa, sb, nu, h, seed)
    assert q.dtype == np.float32 and q.shape == (2 * ns + nu, 3)
    u = q[2 * ns:]
    assert (u >= -h).all() and (u < h).all() and np.array_equal(u, (2 * S.uniforms(seed, nu) - 1) * h)
    # uniform on [-h, h): mean 0 +- h / sqrt(3 n), inside 5 standard errors per coordinate
    assert (np.abs(u.mean(0)) <= 5 * h / np.sqrt(3 * nu)).all()
    z = S.normals(seed, ns, np.float64)
    assert z.shape == (ns, 6) and np.isfinite(z).all()
    # standard normals: the mean's standard error is 1 / sqrt(n), the variance's sqrt(2 / n); pairs of columns uncorrelated (1 / sqrt(n))
    assert (np.abs(z.mean(0)) <= 5 / np.sqrt(ns)).all(), z.mean(0)
    assert (np.abs(z.var(0) - 1) <= 5 * np.sqrt(2.0 / ns)).all(), z.var(0)
    c = np.corrcoef(z.T) - np.eye(6)
    assert np.abs(c).max() <= 5 / np.sqrt(ns), c
    z32 = S.normals(seed, ns)
    assert z32.dtype == np.float32 and np.abs(z32 - z).max() < 1e-5
    assert np.array_equal(q[0:2 * ns:2], surf + sa * z32[:, :3]) and np.array_equal(q[1:2 * ns:2], surf + sb * z32[:, 3:])
    # a pure function of (seed, index): a shorter run is a prefix of each part; another seed differs; the sampler's slots differ
    q2 = S.sdf_queries(surf[:100], sa, sb, 50, h, seed)
    assert np.array_equal(q2[:200], q[:200]) and np.array_equal(q2[200:], u[:50])
    assert not np.array_equal(S.sdf_queries(surf[:100], sa, sb, 50, h, seed + 1), q2)
    from mesh_restatement import rnd_bits
    n = np.arange(4096, dtype=np.uint64)
    mine = set(int(x) for x in rnd_bits(seed, n, 3))
    for k in range(3):
        assert not mine & set(int(x) for x in rnd_bits(seed, n, k))


def test_normalize_to_unit_sphere_and_npz(tmp_path):
    from distr import mesh
    rs = np.random.RandomState(3)
    v = (rs.rand(200, 3) * [4, 2, 1] + [10, -3, 0.5]).astype(np.float32)
    vn, offset, scale = mesh.normalize_to_unit_sphere(v, buffer=1.03)
    assert vn.dtype == np.float32 and vn.shape == v.shape and offset.shape == (3,)
    # the loaders' convention: normalised = (original + offset) * scale; the box centre moves to the origin, the farthest vertex to 1 / buffer
    assert np.abs(vn - (v.astype(np.float64) + offset) * scale).max() <= 2.0 ** -23
    assert np.abs((vn.max(0) + vn.min(0)) / 2).max() <= 1e-6
    assert abs(np.linalg.norm(vn, axis=1).max() * 1.03 - 1) <= 1e-6
    assert np.abs(offset + (v.max(0).astype(np.float64) + v.min(0)) / 2).max() == 0
    pos = rs.randn(7, 4).astype(np.float32)
    neg = -np.abs(rs.randn(5, 4)).astype(np.float32)
    fn = str(tmp_path / 'samples.npz')
    mesh.write_sdf_npz(fn, {'pos': pos, 'neg': neg})
    raw = np.load(fn)
    assert sorted(raw.files) == ['neg', 'pos'] and raw['pos'].dtype == np.float32 and raw['pos'].shape == (7, 4)
    back = mesh.read_sdf_npz(fn)
    assert np.array_equal(back['pos'], pos) and np.array_equal(back['neg'], neg)
