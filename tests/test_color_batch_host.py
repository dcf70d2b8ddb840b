"""CPU-only checks of the batched colour path (SDFRenderer_color.render_batch / relight, decode_color_batch): the
C ABI part against the binding, the argument checks and chunking that need no device, and the shading term of the colour stage with its
four partial derivatives restated in float64 and checked against autograd on the formulas of SDFRenderer_color.compute_shading_maps
(core/sdfrenderer/renderer_rgb.py) -- what the GPU test's comparison with the composed path then rests on."""
import os
import re

import pytest

from conftest import ROOT

SIZES = [1, 64, 65, 0, 130, 63]


def test_color_batch_abi_declared_and_exported():
    from distr import binding
    hdr = open(os.path.join(ROOT, 'include', 'distr_color_batch.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    declared = set(re.findall(r'\b(distr_[a-z0-9_]+)\s*\(', hdr))
    assert declared == set(binding.COLOR_BATCH_EXPORTS)
    top = open(os.path.join(ROOT, 'include', 'distr.h')).read()
    assert '#include "distr_color_batch.h"' in top
    assert re.search(r'#define DISTR_ABI_VERSION 6u', top) and binding.ABI_VERSION == 6          # additive: the ABI version stays
    assert 'distr_color_batch.h' in binding.HEADERS and 'distr_color_batch.hpp' in binding.SOURCES
    binding.build_library()
    L = binding.lib()
    for name in binding.COLOR_BATCH_EXPORTS:               # dlsym
        getattr(L, name)


def test_lights_struct_matches_header():
    import ctypes as C
    from distr import binding
    hdr = open(os.path.join(ROOT, 'include', 'distr_color_batch.h')).read()
    body = re.search(r'typedef struct distr_color_lights \{(.*?)\} distr_color_lights;', hdr, flags=re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    names = [d.strip().split()[-1] for d in body.split(';') if d.strip()]
    assert names == [n for n, _ in binding.ColorLights._fields_]
    assert binding.ColorLights().struct_size == C.sizeof(binding.ColorLights) == 40


def test_workspace_sizes_are_host_code():
    import ctypes as C
    from distr import binding
    binding.build_library()
    L = binding.lib()
    cnt = (C.c_int64 * len(SIZES))(*SIZES)
    f, b = L.distr_color_multi_workspace_bytes(len(SIZES), cnt), L.distr_color_backward_multi_workspace_bytes(len(SIZES), cnt)
    tiles = sum((n + 63) // 64 for n in SIZES)
    assert f >= len(SIZES) * 1024 * 4 and b >= f + tiles * (1024 + 12) * 4
    # the same list layout as the SDF decoder's segmented calls
    assert (f, b) == (L.distr_mlp_multi_workspace_bytes(len(SIZES), cnt), L.distr_mlp_backward_multi_workspace_bytes(len(SIZES), cnt))
    neg = (C.c_int64 * 2)(4, -1)
    for fn in (L.distr_color_multi_workspace_bytes, L.distr_color_backward_multi_workspace_bytes):
        assert fn(0, cnt) == 0 and fn(binding.MAX_SEGMENTS + 1, cnt) == 0 and fn(2, neg) == 0 and fn(2, None) == 0
    assert L.distr_color_eval_multi(None, 1, cnt, None, 0, None, None, None, 0, None) == -1          # no context: DISTR_ERR_INVALID_ARG
    assert L.distr_color_stage_forward_batch(None, None, 1, None, None, None, None, None, None, 0, None, None, None, 0, None, None, None, None) == -1
    assert L.distr_color_relight(None, None, 1, None, None, None, None, None, None, None, None, None) == -1


class _Engine(object):          # what the argument checks of distr.functions read from an engine: a colour decoder with cs = 8
    latent_size = 256 + 8

    def __init__(self):
        import torch
        self.device = torch.device('cpu')


def test_code_rows_and_their_errors():
    import torch
    from distr import functions
    eng = _Engine()
    sc, cc = torch.arange(3 * 256, dtype=torch.float32).reshape(3, 256), -torch.arange(3 * 8, dtype=torch.float32).reshape(3, 8)
    rows = functions.color_code_rows(eng, cc, sc, 3)
    assert rows.shape == (3, 264) and torch.equal(rows[:, :256], sc) and torch.equal(rows[:, 256:], cc)         # [shape | colour]
    assert functions.color_code_rows(eng, cc[:1], sc[:1], 3).shape == (1, 264)                                 # both shared: one row, stride 0
    mixed = functions.color_code_rows(eng, cc[:1], sc, 3)                                                      # a shared colour code, a shape code per view
    assert mixed.shape == (3, 264) and torch.equal(mixed[:, 256:], cc[:1].expand(3, -1)) and torch.equal(mixed[:, :256], sc)
    for bad_c, bad_s in ((cc[:, :7], sc), (cc, sc[:, :255]), (cc[:2], sc), (cc, sc[:2]), (cc.reshape(-1), sc)):
        with pytest.raises(ValueError, match=r'shape codes \(1, 256\) or \(3, 256\) and colour codes \(1, 8\) or \(3, 8\)'):
            functions.color_code_rows(eng, bad_c, bad_s, 3)
    # a code gradient's rows go back to the inputs' shapes; a shared code gets the sum of the rows
    g = torch.arange(3 * 264, dtype=torch.float32).reshape(3, 264)
    g_c, g_s = functions._split_code_grad(g, cc[:1], sc)
    assert torch.equal(g_c, g[:, 256:].sum(0, keepdim=True)) and torch.equal(g_s, g[:, :256])


def test_chunks_of_64_segments():
    """decode_color_batch cuts longer lists into chunks of 64 segments exactly as decode_sdf_batch does: the same plan, the code rows
    of a chunk starting at its first segment (or row 0 with stride 0 for a shared pair)."""
    import torch
    from distr import functions
    eng = _Engine()
    plan = functions.segment_plan([3] * 65)
    assert plan['chunks'] == [(0, 64), (64, 65)]
    rows = functions.color_code_rows(eng, torch.zeros(65, 8), torch.zeros(1, 256), 65)
    assert list(functions._multi_chunks(rows, plan)) == [(0, 64, 0, 0, 264), (64, 1, 192, 64, 264)]
    rows = functions.color_code_rows(eng, torch.zeros(1, 8), torch.zeros(1, 256), 65)
    assert list(functions._multi_chunks(rows, plan)) == [(0, 64, 0, 0, 0), (64, 1, 192, 0, 0)]
    lat, x, p2 = functions._multi_args(eng, rows, torch.zeros(195, 3), [3] * 65)
    assert lat.shape == (1, 264) and x.shape == (195, 3) and p2['total'] == 195


def test_decode_color_batch_argument_errors():
    import torch
    from core.utils import decoder_utils as du
    cc, sc = torch.zeros(len(SIZES), 8), torch.zeros(len(SIZES), 256)
    pts = torch.zeros(sum(SIZES), 3)
    x, counts, shape = du._color_batch_layout(cc, sc, pts, SIZES)
    assert x.shape == (323, 3) and counts == SIZES and shape == (323,)
    assert du._color_batch_layout(cc[:1], sc[:1], pts, torch.tensor(SIZES))[1] == SIZES                    # shared codes, a CPU int tensor
    x, counts, shape = du._color_batch_layout(cc[:3], sc[:1], torch.zeros(3, 5, 3), None)
    assert x.shape == (15, 3) and counts == [5, 5, 5] and shape == (3, 5)
    with pytest.raises(ValueError, match=r'color_codes has shape \(5, 8\); 6 segments take \(1, C\) \(shared\) or \(6, C\)'):
        du._color_batch_layout(cc[:5], sc, pts, SIZES)
    with pytest.raises(ValueError, match=r'shape_codes has shape \(2, 256\)'):
        du._color_batch_layout(cc, sc[:2], pts, SIZES)
    with pytest.raises(ValueError, match='counts sum to 324, but there are 323 points'):
        du._color_batch_layout(cc, sc, pts, [2] + SIZES[1:])
    with pytest.raises(ValueError, match='segment sizes'):
        du._color_batch_layout(cc, sc, pts, [-1, 66] + SIZES[2:])
    with pytest.raises(ValueError, match='at least one segment'):
        du._color_batch_layout(cc, sc, pts[:0], [])
    with pytest.raises(ValueError, match=r'\(S, N, 3\)'):
        du._color_batch_layout(cc, sc, pts, None)                      # a flat list without counts
    with pytest.raises(ValueError, match='flat list'):
        du._color_batch_layout(cc[:3], sc[:3], torch.zeros(3, 5, 3), [5, 5, 5])
    with pytest.raises(RuntimeError, match='must be on the GPU'):      # CPU tensors raise as decode_color does
        du.decode_color_batch(None, cc, sc, pts, counts=SIZES)


def test_lights_argument_checks():
    import torch
    from distr import functions
    dev = torch.device('cpu')
    assert functions.color_lights(dev, 4, None, None) == (None, None, None)
    loc, en, st = functions.color_lights(dev, 4, torch.zeros(3, 3), None)
    assert loc.shape == (3, 3) and torch.equal(en, torch.ones(3)) and (st.nlights, st.location_stride, st.energy_stride) == (3, 0, 0)
    loc, en, st = functions.color_lights(dev, 4, torch.zeros(4, 3, 3), torch.ones(4, 3))
    assert (st.nlights, st.location_stride, st.energy_stride) == (3, 9, 3) and st.locations_dev == loc.data_ptr() and st.energies_dev == en.data_ptr()
    assert functions.color_lights(dev, 4, torch.zeros(4, 3, 3), torch.ones(3))[2].energy_stride == 0
    for bad in (torch.zeros(3), torch.zeros(3, 2), torch.zeros(5, 3, 3), torch.zeros(0, 3)):
        with pytest.raises(ValueError, match=r'expected \(M, 3\) or \(4, M, 3\)'):
            functions.color_lights(dev, 4, bad, None)
    with pytest.raises(ValueError, match=r'expected \(3,\) or \(4, 3\)'):
        functions.color_lights(dev, 4, torch.zeros(3, 3), torch.ones(2))
    with pytest.raises(ValueError, match='lighting_locations requires grad'):
        functions.color_lights(dev, 4, torch.zeros(3, 3, requires_grad=True), None)
    with pytest.raises(ValueError, match='lighting_energies requires grad'):
        functions.color_lights(dev, 4, torch.zeros(3, 3), torch.ones(3, requires_grad=True))


# ---- the shading term and its partial derivatives as the colour stage computes them (csrc/distr_color_batch.hpp), in float64
def shading_restated(R, q, n, lights, energies):
    """s[i] = sum_m e_m ((R l_m) . n_i), l_m = (L_m - q_i) / |L_m - q_i|: q (N,3) the surface points WITHOUT the inverse transform, n (N,3)
    the transformed normals, lights (M,3), energies (M,). Returns (s (N,), l (M,N,3), 1 / |L_m - q| (M,N))."""
    import torch
    u = lights[:, None, :] - q[None, :, :]
    inv = 1.0 / u.norm(dim=2)
    l = u * inv[:, :, None]
    lam = ((l @ R.t()) * n[None]).sum(2)                   # rows of l @ R^T = R l
    return (energies[:, None] * lam).sum(0), l, inv


def shading_backward_restated(R, q, n, lights, energies, color, g_rgb):
    """The four partial derivatives of  rgb = color * s  for the upstream gradient g_rgb (N,3): (g_color = g_rgb s; g_n = g_s sum_m e_m R l_m;
    the explicit g_R[j][k] = sum_i g_s sum_m e_m n_j l_k; g_q = -sum_m (g_l - l (l . g_l)) / |L_m - q| with g_l = g_s e_m R^T n), where
    g_s = sum_c g_rgb_c color_c."""
    import torch
    s, l, inv = shading_restated(R, q, n, lights, energies)
    gs = (g_rgb * color).sum(1)                                                        # (N,)
    g_color = g_rgb * s[:, None]
    g_n = gs[:, None] * (energies[:, None, None] * (l @ R.t())).sum(0)
    g_R = torch.einsum('i,m,ij,mik->jk', gs, energies, n, l)
    gl = gs[None, :, None] * energies[:, None, None] * (n @ R)[None]                   # (M,N,3): R^T n per pixel
    g_q = -((gl - l * (l * gl).sum(2, keepdim=True)) * inv[:, :, None]).sum(0)
    return g_color, g_n, g_R, g_q


@pytest.mark.parametrize('M', [1, 3])
def test_shading_term_and_derivatives_against_autograd(M):
    """The composed path's formulas (SDFRenderer_color.compute_shading_maps and the `color * shading` of render, renderer_rgb.py) under
    autograd, in float64, against the restatement above: the value and all four partial derivatives."""
    import torch
    torch.manual_seed(7 + M)
    N = 37
    f64 = dict(dtype=torch.float64)
    A = torch.randn(3, 3, **f64)
    R = torch.linalg.qr(A)[0].requires_grad_(True)
    q = (0.4 * torch.randn(N, 3, **f64)).requires_grad_(True)
    n = torch.nn.functional.normalize(torch.randn(N, 3, **f64), dim=1).requires_grad_(True)
    color = torch.rand(N, 3, **f64).requires_grad_(True)
    lights = 2.0 * torch.randn(M, 3, **f64) + torch.tensor([0.0, 0.0, 3.0], **f64)
    energies = 0.5 + torch.rand(M, **f64)
    g_rgb = torch.randn(N, 3, **f64)
    # renderer_rgb.py: to_light = L - pts; normalise; z_dirs = to_light @ R^T; lambert = (z_dirs * n).sum; shading = (lambert * e).sum(0)
    to_light = lights[:, None, :] - q[None, :, :]
    to_light = to_light / torch.norm(to_light, p=2, dim=2, keepdim=True)
    z_dirs = torch.matmul(to_light, R.t())
    lambert = (z_dirs * n[None]).sum(2)
    shading = (lambert * energies[:, None]).sum(0)
    rgb = color * shading[:, None]
    rgb.backward(g_rgb)
    with torch.no_grad():
        s, _, _ = shading_restated(R, q, n, lights, energies)
        g_color, g_n, g_R, g_q = shading_backward_restated(R, q, n, lights, energies, color, g_rgb)
    assert torch.allclose(s, shading.detach(), rtol=1e-12, atol=1e-13)
    for name, got, want in (('g_color', g_color, color.grad), ('g_n', g_n, n.grad), ('g_R', g_R, R.grad), ('g_q', g_q, q.grad)):
        assert float(want.abs().max()) > 0, name
        assert torch.allclose(got, want, rtol=1e-10, atol=1e-12 * float(want.abs().max())), name
