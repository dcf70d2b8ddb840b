"""CPU-only checks of the depth-samples part of the C ABI (include/distr_samples.h) against the binding, and of golden G31's own
consistency."""
import ctypes as C
import os
import re

import numpy as np

from conftest import GOLDEN, ROOT


def test_samples_abi_declared_exported_and_checked():
    from distr import binding
    hdr = open(os.path.join(ROOT, 'include', 'distr_samples.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    declared = set(re.findall(r'\b(distr_[a-z0-9_]+)\s*\(', hdr))
    assert declared == set(binding.SAMPLES_EXPORTS)
    assert '#include "distr_samples.h"' in open(os.path.join(ROOT, 'include', 'distr.h')).read()
    assert 'DISTR_ABI_VERSION 6u' in open(os.path.join(ROOT, 'include', 'distr.h')).read() and binding.ABI_VERSION == 6
    binding.build_library()
    L = binding.lib()
    for name in binding.SAMPLES_EXPORTS:             # dlsym
        assert hasattr(L, name), name
    # the struct the binding mirrors: struct_size, H, W, K_inv[9], M[9], clamp_dist, mode, number
    assert C.sizeof(binding.SamplesCfg) == 4 * (3 + 9 + 9 + 3)
    # calls without a context are refused, not crashed
    cfg = binding.make_samples_cfg((8, 8), np.eye(3), np.eye(3), 0.1, 'surface')
    assert cfg.struct_size == C.sizeof(binding.SamplesCfg) and cfg.mode == 0
    assert binding.make_samples_cfg((8, 8), np.eye(3), np.eye(3), None, 'freespace', 3).clamp_dist == -1.0
    nb = C.c_size_t()
    assert L.distr_depth_samples_workspace_bytes(None, C.byref(cfg), 1, None, C.byref(nb), None, None) == -1
    assert L.distr_depth_samples_count(None, C.byref(cfg), 1, None, None, None, None, 0, None) == -1


def test_samples_cfg_struct_size_handshake():
    """distr_depth_samples_workspace_bytes with counts = NULL is host code: a context created without a device still answers it (as
    distr_workspace_bytes does in test_host_logic.py::test_abi_handshake). A good cfg gets a size; a zeroed, a short and a longer
    struct are refused before any field is read; so are 65 views and number = 0."""
    from distr import binding
    binding.build_library()
    L = binding.lib()
    h = C.c_void_p()
    L.distr_create_abi(C.byref(h), 0, binding.ABI_VERSION)          # (fails for lack of a device; the context still answers)
    K = np.array([[48., 0, 24], [0, 40., 20], [0, 0, 1]])
    cfg = binding.make_samples_cfg((40, 48), K, np.eye(3), 0.1, 'surface')
    assert cfg.struct_size == C.sizeof(binding.SamplesCfg) and binding.SamplesCfg._fields_[0][0] == 'struct_size'
    nb = C.c_size_t()
    wsb = lambda c, nviews=1: L.distr_depth_samples_workspace_bytes(h, C.byref(c), nviews, None, C.byref(nb), None, None)
    assert wsb(cfg) == 0 and nb.value > 0
    one = nb.value
    assert wsb(cfg, 64) == 0 and nb.value >= one
    good = cfg.struct_size
    for bad in (0, good - 4, good + 8):
        cfg.struct_size = bad
        assert wsb(cfg) == -1, bad
        assert b'struct_size' in L.distr_last_error(h)
    cfg.struct_size = good
    assert wsb(cfg) == 0
    assert wsb(cfg, 65) == -1 and b'nviews' in L.distr_last_error(h)
    assert wsb(cfg, 0) == -1
    free = binding.make_samples_cfg((40, 48), K, np.eye(3), 0.1, 'freespace', number=0)
    assert wsb(free) == -1 and b'number' in L.distr_last_error(h)
    free.number = binding.SAMPLES_MAX_NUMBER + 1
    assert wsb(free) == -1
    free.number = binding.SAMPLES_MAX_NUMBER
    assert wsb(free) == 0
    free.mode = 7
    assert wsb(free) == -1 and b'mode' in L.distr_last_error(h)
    # the forward / backward sizes need the counts
    fb = C.c_size_t()
    assert L.distr_depth_samples_workspace_bytes(h, C.byref(cfg), 1, None, None, C.byref(fb), None) == -1
    cnt = (C.c_int64 * 1)(40 * 48 + 1)
    assert L.distr_depth_samples_workspace_bytes(h, C.byref(cfg), 1, cnt, None, C.byref(fb), None) == -1      # more than H * W
    cnt[0] = 500
    bb = C.c_size_t()
    assert L.distr_depth_samples_workspace_bytes(h, C.byref(cfg), 1, cnt, None, C.byref(fb), C.byref(bb)) == 0 and 0 < fb.value < bb.value
    L.distr_destroy(h)


def test_binding_constants_match_the_header():
    from distr import binding
    hdr = open(os.path.join(ROOT, 'include', 'distr_samples.h')).read()
    top = open(os.path.join(ROOT, 'include', 'distr.h')).read()
    define = lambda text, name: int(re.search(r'#define %s (\d+)' % name, text).group(1))
    assert define(hdr, 'DISTR_SAMPLES_SURFACE') == binding.SAMPLES_MODES['surface']
    assert define(hdr, 'DISTR_SAMPLES_FREESPACE') == binding.SAMPLES_MODES['freespace']
    assert define(hdr, 'DISTR_SAMPLES_MAX_NUMBER') == binding.SAMPLES_MAX_NUMBER
    assert define(top, 'DISTR_MAX_VIEWS') == binding.MAX_VIEWS
    # field order and types of distr_samples_cfg against the ctypes mirror
    body = re.sub(r'/\*.*?\*/', '', re.search(r'typedef struct distr_samples_cfg \{(.*?)\} distr_samples_cfg;', hdr, flags=re.S).group(1), flags=re.S)
    fields = []
    for decl in [d.strip() for d in body.split(';') if d.strip()]:
        ctype, names = decl.split(None, 1)
        for nme in names.split(','):
            m = re.match(r'\s*(\w+)(?:\[(\d+)\])?\s*$', nme)
            fields.append((m.group(1), ctype, int(m.group(2) or 0)))
    base = {'uint32_t': C.c_uint32, 'int32_t': C.c_int32, 'float': C.c_float}
    want = [(n, base[t] * k if k else base[t]) for n, t, k in fields]
    assert [(n, t) for n, t in binding.SamplesCfg._fields_] == want


def test_g31_loads_and_is_consistent():
    g = dict(np.load(os.path.join(GOLDEN, 'g31_depth_samples.npz')))
    assert os.path.getsize(os.path.join(GOLDEN, 'g31_depth_samples.npz')) < 1 << 20
    assert all(a.dtype.kind in 'fiuU' for a in g.values())          # arrays and short key strings only
    for fx in [str(f) for f in g['fixtures']]:
        depth = g[fx + '_depth']
        assert depth.shape == (int(g['H']), int(g['W'])) and g[fx + '_normal'].shape == depth.shape + (3,)
        N = int(g[fx + '_N'])
        assert N == int(((depth > 0) & (depth < 1e5)).sum()) and N > 0
        for name in [str(c) for c in g['case_names']]:
            key = '%s_%s_' % (fx, name)
            clamp = float(g[key + 'clamp_dist'])
            out = g[key + 'out']
            if name.startswith('s_'):
                eta = g[key + 'eta_map']
                assert eta.shape == (N,) and out.shape == (2 * N,) and eta.min() >= 0 and eta.max() <= float(g['eta'])
                pos, neg = out[:N] + eta, out[N:] - eta           # the clamped decoder outputs
                assert np.abs(pos).max() <= clamp + 1e-6 and np.abs(neg).max() <= clamp + 1e-6
            else:
                ratio = g[key + 'ratio']
                assert ratio.shape[1] == N and out.shape == (ratio.shape[0] * N,) and ratio.min() >= 0 and ratio.max() < 1
                assert np.abs(out).max() <= clamp + 1e-6
            assert g[key + 'w'].shape == out.shape and g[key + 'g_points'].shape == out.shape + (3,)
            assert g[key + 'g_latent'].shape == g[fx + '_latent'].shape and g[key + 'g_RT'].shape == (3, 4)
            for k in ('out', 'g_latent_rel', 'g_R_rel', 'g_T_rel'):
                assert 0 < float(g[key + 'floor_' + k]) < 1e-2
