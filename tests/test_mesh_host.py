"""CPU-only checks of shape evaluation: the mesh part of the C ABI (include/distr_mesh.h) against the binding, the numpy PLY writer /
reader, and how core.evaluation resolves Evaluator / latent_vec_to_points / the chamfer functions with and without a reference
checkout next to this build."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG, ROOT


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
