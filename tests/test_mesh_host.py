"""CPU-only checks of shape evaluation: the mesh part of the C ABI (include/distr_mesh.h) against the binding, the numpy PLY writer /
reader, how core.evaluation resolves Evaluator / latent_vec_to_points / the chamfer functions with and without a reference
checkout next to this build, and the numpy restatements (tests/mesh_restatement.py) that tests/test_gpu_mesh.py compares the sampling
and nearest-distance kernels with bit for bit: checked here against independent statements of the same thing."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG, ROOT
import mesh_restatement as R


def test_mesh_abi_declared_exported_and_checked():
    from distr import binding
    hdr = open(os.path.join(ROOT, 'include', 'distr_mesh.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    declared = set(re.findall(r'\b(distr_[a-z0-9_]+)\s*\(', hdr))
    assert declared == set(binding.MESH_EXPORTS)
    assert '#include "distr_mesh.h"' in open(os.path.join(ROOT, 'include', 'distr.h')).read()
    binding.build_library()
    L = binding.lib()
    for name in binding.MESH_EXPORTS:
        assert hasattr(L, name), name
    # GPU-free calls: refused grids have no workspace, sizes grow with the grid
    assert L.distr_mc_workspace_bytes(1, 8, 8) == 0 and L.distr_mc_workspace_bytes(8, 8, 1) == 0
    assert L.distr_mc_workspace_bytes(2048, 1024, 1024) == 0                    # 2^31 values
    assert 0 < L.distr_mc_workspace_bytes(2, 2, 2) < L.distr_mc_workspace_bytes(64, 64, 64)
    assert L.distr_mc_workspace_bytes(64, 64, 64) >= 64 ** 3 * 14
    assert L.distr_sample_workspace_bytes(0) == 0 and L.distr_sample_workspace_bytes(1000) >= 8000
    assert L.distr_nearest_workspace_bytes(0) > 0
    # calls without a context are refused, not crashed
    assert L.distr_mc_count(None, None, 8, 8, 8, 0.0, None, None, None, 0, None) == -1


def test_ply_round_trip_and_layout(tmp_path):
    from distr import mesh
    rs = np.random.RandomState(0)
    v = rs.randn(7, 3).astype(np.float32)
    f = rs.randint(0, 7, (5, 3)).astype(np.int32)
    fn = str(tmp_path / 'm.ply')
    mesh.write_ply(fn, v, f)
    data = open(fn, 'rb').read()
    header = (b'ply\nformat binary_little_endian 1.0\nelement vertex 7\nproperty float x\nproperty float y\nproperty float z\n'
              b'element face 5\nproperty list uchar int vertex_indices\nend_header\n')
    assert data.startswith(header) and len(data) == len(header) + 7 * 12 + 5 * 13
    body = data[len(header):]
    assert body[:12] == v[0].astype('<f4').tobytes() and body[84:85] == b'\x03' and body[85:97] == f[0].astype('<i4').tobytes()
    rv, rf = mesh.read_ply(fn)
    assert rv.dtype == np.float32 and rf.dtype == np.int32
    assert np.array_equal(rv, v) and np.array_equal(rf, f)
    mesh.write_ply(fn, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    rv, rf = mesh.read_ply(fn)
    assert rv.shape == (0, 3) and rf.shape == (0, 3)
    # a PLY with more vertex properties (normals, doubles) and an int8 list count still reads
    hdr = (b'ply\nformat binary_little_endian 1.0\nelement vertex 3\nproperty double x\nproperty double y\nproperty double z\n'
           b'property float nx\nelement face 1\nproperty list char uint vertex_indices\nend_header\n')
    vr = np.zeros(3, dtype=[('x', '<f8'), ('y', '<f8'), ('z', '<f8'), ('nx', '<f4')])
    vr['x'], vr['y'], vr['z'] = [1, 2, 3], [4, 5, 6], [7, 8, 9]
    fr = np.zeros(1, dtype=[('n', 'i1'), ('i', '<u4', (3,))])
    fr['n'], fr['i'] = 3, [[2, 1, 0]]
    open(fn, 'wb').write(hdr + vr.tobytes() + fr.tobytes())
    rv, rf = mesh.read_ply(fn)
    assert np.array_equal(rv, [[1, 4, 7], [2, 5, 8], [3, 6, 9]]) and np.array_equal(rf, [[2, 1, 0]])
    open(fn, 'wb').write(b'ply\nformat ascii 1.0\nend_header\n')
    with pytest.raises(ValueError):
        mesh.read_ply(fn)


_WHERE = r'''
import inspect, json, os, sys
from core.evaluation import *
import core.evaluation as ce
w = lambda o: os.path.abspath(inspect.getsourcefile(o))
ev_mod = sys.modules[Evaluator.__module__]
g = lambda n: w(getattr(ev_mod, n)) if hasattr(ev_mod, n) else None
print(json.dumps({'Evaluator': w(Evaluator), 'latent_vec_to_points': w(latent_vec_to_points),
                  'compute_chamfer_distance': w(compute_chamfer_distance),
                  'compute_chamfer_distance_separate': w(compute_chamfer_distance_separate),
                  'ev.latent_vec_to_points': g('latent_vec_to_points'), 'ev.compute_chamfer_distance': g('compute_chamfer_distance'),
                  'ev.compute_chamfer_distance_separate': g('compute_chamfer_distance_separate'),
                  'ev.create_mesh': g('create_mesh'), 'ev.decode_sdf': g('decode_sdf'),
                  'methods': sorted(n for n in vars(Evaluator) if not n.startswith('_')),
                  'all': sorted(n for n in ('Evaluator', 'latent_vec_to_points', 'compute_chamfer_distance', 'compute_chamfer_distance_separate',
                                            'sample_points_from_ply_file', 'create_mesh', 'create_mesh_speedup') if n in ce.__all__)}))
'''


def _where(pythonpath):
    out = subprocess.run([sys.executable, '-c', _WHERE], env=dict(os.environ, PYTHONPATH=os.pathsep.join(pythonpath)), capture_output=True,
                         text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    return json.loads([l for l in out.stdout.splitlines() if l.startswith('{')][-1])


def test_evaluation_names_without_a_reference_checkout():
    j = _where([PKG])
    ours = os.path.join(PKG, 'core', 'evaluation')
    assert j['Evaluator'] == os.path.join(ours, 'gpu_evaluator.py')
    for k in ('latent_vec_to_points', 'ev.latent_vec_to_points'):
        assert j[k] == os.path.join(ours, 'transforms.py'), k
    for k in ('compute_chamfer_distance', 'compute_chamfer_distance_separate', 'ev.compute_chamfer_distance'):
        assert j[k] == os.path.join(ours, 'eval_func.py'), k
    assert j['methods'] == ['compute_chamfer_distance', 'latent_vec_to_points']
    assert j['all'] == ['Evaluator', 'compute_chamfer_distance', 'compute_chamfer_distance_separate', 'create_mesh', 'create_mesh_speedup',
                        'latent_vec_to_points', 'sample_points_from_ply_file']


_CHECKOUT = {
    'core/__init__.py': "raise AssertionError('checkout core/__init__.py executed')\n",
    'core/evaluation/__init__.py': "raise AssertionError('checkout core/evaluation/__init__.py executed')\n",
    'core/evaluation/evaluator.py': ("import os, sys\nsys.path.append(os.path.dirname(os.path.abspath(__file__)))\nimport torch\n"
                                     "from eval_func import *\nfrom transforms import *\n\n\nclass Evaluator(object):\n"
                                     "    def __init__(self, decoder):\n        self.decoder = decoder\n"),
    'core/evaluation/eval_func.py': "raise AssertionError('checkout eval_func.py imported: needs scipy')\n",
    'core/evaluation/transforms.py': "raise AssertionError('checkout transforms.py imported: needs trimesh')\n",
    'core/evaluation/create_mesh.py': "raise AssertionError('checkout create_mesh.py imported: needs scikit-image')\n",
}


def test_reference_checkout_evaluator_lands_on_this_build(tmp_path):
    """A checkout shaped like the reference's (evaluator.py: `from eval_func import *; from transforms import *`): its Evaluator is
    re-exported, and the flat names it star-imports are this build's GPU functions (the checkout's own files would raise)."""
    for rel, text in _CHECKOUT.items():
        p = tmp_path / rel
        p.parent.mkdir(parents=True, exist_ok=True)
        p.write_text(text)
    j = _where([PKG, str(tmp_path)])
    ours = os.path.join(PKG, 'core')
    assert j['Evaluator'] == str(tmp_path / 'core' / 'evaluation' / 'evaluator.py')
    for k in ('latent_vec_to_points', 'ev.latent_vec_to_points', 'compute_chamfer_distance', 'ev.compute_chamfer_distance',
              'ev.compute_chamfer_distance_separate', 'ev.create_mesh', 'ev.decode_sdf'):
        assert j[k].startswith(ours), (k, j[k])
    assert j['ev.latent_vec_to_points'] == os.path.join(ours, 'evaluation', 'transforms.py')
    assert j['ev.decode_sdf'] == os.path.join(ours, 'utils', 'decoder_utils.py')


# ------------------------------------------------------------------------------------------------ restatements of the mesh kernels
_M = 2 ** 64 - 1


def _mix64_int(z):
    z = (z + 0x9E3779B97F4A7C15) & _M
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M
    return z ^ (z >> 31)


def test_rnd_bits_restatement_against_python_ints():
    assert int(R.mix64(0)[0]) == 0xE220A8397B1DCDAF                  # the first output of SplitMix64 seeded with 0
    assert _mix64_int(0) == 0xE220A8397B1DCDAF
    cases = [(0, 0, 0), (5, 1, 2), (2 ** 64 - 1, 7, 1), (2 ** 64 - 1, 2 ** 40 - 1, 2), (12345678901234567, 2 ** 40 + 3, 0),
             (1, 2 ** 40, 1), (2 ** 63, 99999, 2), (6, 2 ** 62 - 1, 2)]      # the last: 4 * i + k wraps nowhere yet, just below 2^64
    for seed, i, k in cases:
        want = _mix64_int(_mix64_int(seed) ^ _mix64_int((4 * i + k) & _M))
        assert int(R.rnd_bits(seed, i, k)[0]) == want, (seed, i, k)
    i = np.array([c[1] for c in cases], dtype=np.uint64)
    got = R.rnd_bits(2 ** 64 - 1, i, 1)
    assert [int(x) for x in got] == [_mix64_int(_mix64_int(_M) ^ _mix64_int((4 * int(j) + 1) & _M)) for j in i]


def test_nearest_restatement_against_float64():
    """Three roundings of relative size u = 2^-24 on the differences, three on the squares, two on the sums: at most 5u to first order
    on every candidate, and the minimum keeps a relative bound. Coordinates of ordinary magnitude, so no term is subnormal."""
    rs = np.random.RandomState(4)
    A = rs.randn(700, 3).astype(np.float32)
    B = (rs.randn(1900, 3) * 0.8).astype(np.float32)
    B[:50] = A[:50] + (rs.randn(50, 3) * 1e-3).astype(np.float32)      # close pairs, where an expansion of |a - b|^2 cancels
    got = R.nearest_sq_dist_f32(A, B)
    assert got.dtype == np.float32 and got.shape == (700,)
    assert np.array_equal(got, R.nearest_sq_dist_f32(A, B, max_elems=4001))         # the row chunks do not matter
    d = A.astype(np.float64)[:, None, :] - B.astype(np.float64)[None, :, :]
    want = (d * d).sum(2).min(1)
    assert want.min() > 1e-12
    assert (np.abs(got.astype(np.float64) - want) <= 6 * 2.0 ** -24 * want).all()
    assert R.nearest_sq_dist_f32(B[:3], B)[1] == 0.0


def test_sample_surface_restatement_on_two_triangles():
    """Two triangles of areas 3 and 1 in the plane z = 1: face frequencies inside 5 sigma, every point inside its triangle. The
    barycentric coordinates solve [a b c] l = p (the plane misses the origin, so the system is regular): their sum tells whether the
    point is in the plane. Float32 rounding of the point puts a coordinate up to about 1e-7 outside, hence 1e-6 on both checks."""
    v = np.array([[0, 0, 1], [2, 0, 1], [0, 3, 1], [5, 5, 1], [6, 5, 1], [5, 7, 1]], np.float32)
    f = np.array([[0, 1, 2], [3, 4, 5]], np.int32)
    n = 200000
    p, fi, band = R.sample_surface(v, f, n, 9)
    assert p.dtype == np.float32 and p.shape == (n, 3) and fi.shape == (n,) and band.shape == (n,) and (band >= 0).all()
    hits = np.bincount(fi, minlength=2)
    assert abs(hits[0] - 0.75 * n) <= 5 * np.sqrt(n * 0.75 * 0.25), hits
    for k in range(2):
        m = v[f[k]].astype(np.float64).T                              # columns a, b, c
        lam = np.linalg.solve(m, p[fi == k].astype(np.float64).T).T
        assert lam.min() >= -1e-6 and np.abs(lam.sum(1) - 1).max() <= 1e-6, (k, lam.min())
        assert np.abs(lam.mean(0) - 1.0 / 3).max() < 5e-3              # uniform inside the triangle
    # a pure function of (seed, index): a shorter run is a prefix, another seed differs
    q, qi, _ = R.sample_surface(v, f, 1000, 9)
    assert np.array_equal(q, p[:1000]) and np.array_equal(qi, fi[:1000])
    assert not np.array_equal(R.sample_surface(v, f, 1000, 10)[0], q)
    # a face of area 0 or naming a vertex outside the array is never picked
    f3 = np.array([[0, 1, 2], [0, 0, 1], [0, 1, 6], [-1, 1, 2], [3, 4, 5], [3, 3, 3]], np.int32)
    _, fi3, _ = R.sample_surface(v, f3, 20000, 1)
    assert set(np.unique(fi3)) == {0, 4}
