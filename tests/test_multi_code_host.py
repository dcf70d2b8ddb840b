"""CPU-only checks of the segmented point list (decode_sdf_batch): the C ABI part against the binding, the
host-side plan (segment offsets, tiles per segment, chunks of 64 segments) and the argument errors of the Python layer."""
import os
import re

import pytest

from conftest import ROOT

SIZES = [1, 64, 65, 0, 130, 63]


def test_multi_abi_declared_and_exported():
    from distr import binding
    hdr = open(os.path.join(ROOT, 'include', 'distr_multi.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    declared = set(re.findall(r'\b(distr_[a-z0-9_]+)\s*\(', hdr))
    assert declared == set(binding.MULTI_EXPORTS)
    assert '#include "distr_multi.h"' in open(os.path.join(ROOT, 'include', 'distr.h')).read()
    assert re.search(r'#define DISTR_ABI_VERSION %du' % binding.ABI_VERSION, open(os.path.join(ROOT, 'include', 'distr.h')).read())
    binding.build_library()
    L = binding.lib()
    for name in binding.MULTI_EXPORTS:               # dlsym
        getattr(L, name)
    assert 'distr_multi.h' in binding.HEADERS


def test_workspace_sizes_are_host_code():
    """The *_workspace_bytes of the segmented calls need no context: 0 for what the calls refuse, else growing with segments and tiles."""
    import ctypes as C
    from distr import binding
    binding.build_library()
    L = binding.lib()
    cnt = (C.c_int64 * len(SIZES))(*SIZES)
    f, b = L.distr_mlp_multi_workspace_bytes(len(SIZES), cnt), L.distr_mlp_backward_multi_workspace_bytes(len(SIZES), cnt)
    tiles = sum((n + 63) // 64 for n in SIZES)
    assert f >= len(SIZES) * 1024 * 4 and b >= f + tiles * (1024 + 12) * 4
    assert L.distr_mlp_multi_workspace_bytes(1, (C.c_int64 * 1)(8)) < f
    neg = (C.c_int64 * 2)(4, -1)
    for fn in (L.distr_mlp_multi_workspace_bytes, L.distr_mlp_backward_multi_workspace_bytes):
        assert fn(0, cnt) == 0 and fn(binding.MAX_SEGMENTS + 1, cnt) == 0 and fn(2, neg) == 0 and fn(2, None) == 0
    assert L.distr_mlp_eval_multi(None, 1, cnt, None, 0, None, 0.1, None, None, 0, None) == -1       # no context: DISTR_ERR_INVALID_ARG


def test_segment_plan():
    from distr import binding, functions
    assert binding.MAX_SEGMENTS == 64 and binding.SEG_TILE == 64
    p = functions.segment_plan(SIZES)
    assert p['offsets'] == [0, 1, 65, 130, 130, 260]
    assert p['tiles'] == [1, 1, 2, 0, 3, 1]              # every segment rounds up on its own; the empty one gets no tile
    assert p['total'] == 323 and p['chunks'] == [(0, 6)]
    p = functions.segment_plan([3] * 65)
    assert p['chunks'] == [(0, 64), (64, 65)] and p['offsets'][64] == 192 and p['tiles'] == [1] * 65 and p['total'] == 195
    assert functions.segment_plan([0] * 128)['chunks'] == [(0, 64), (64, 128)]
    assert functions.segment_plan([64])['tiles'] == [1] and functions.segment_plan([4097])['tiles'] == [65]
    with pytest.raises(ValueError):
        functions.segment_plan([])
    with pytest.raises(ValueError):
        functions.segment_plan([4, -1])


class _Engine(object):          # what the argument checks of distr.functions read from an engine
    latent_size = 8

    def __init__(self):
        import torch
        self.device = torch.device('cpu')


def test_functions_argument_errors():
    import torch
    from distr import functions
    eng = _Engine()
    pts = torch.zeros(sum(SIZES), 3)
    lat, x, plan = functions._multi_args(eng, torch.zeros(len(SIZES), 8), pts, SIZES)
    assert lat.shape == (len(SIZES), 8) and x.shape == (323, 3) and plan['total'] == 323
    assert functions._multi_args(eng, torch.zeros(1, 8), pts, SIZES)[0].shape == (1, 8)          # one shared code
    with pytest.raises(ValueError, match=r'\(S, C\) = \(6, 8\)'):
        functions._multi_args(eng, torch.zeros(len(SIZES), 9), pts, SIZES)
    with pytest.raises(ValueError, match=r'\(S, C\) = \(6, 8\)'):
        functions._multi_args(eng, torch.zeros(5, 8), pts, SIZES)
    with pytest.raises(ValueError, match='counts sum to 323, but there are 300 points'):
        functions._multi_args(eng, torch.zeros(len(SIZES), 8), pts[:300], SIZES)
    # chunks of a 65-segment call: (first segment, segments, first point, code row, latent_stride), per-segment codes and one shared code
    plan = functions.segment_plan([3] * 65)
    assert list(functions._multi_chunks(torch.zeros(65, 8), plan)) == [(0, 64, 0, 0, 8), (64, 1, 192, 64, 8)]
    assert list(functions._multi_chunks(torch.zeros(1, 8), plan)) == [(0, 64, 0, 0, 0), (64, 1, 192, 0, 0)]


def test_decode_sdf_batch_argument_errors():
    import torch
    from core.utils import decoder_utils as du
    Cn = 8
    lat = torch.zeros(len(SIZES), Cn)
    pts = torch.zeros(sum(SIZES), 3)
    x, counts, shape = du._batch_layout(Cn, lat, pts, SIZES)
    assert x.shape == (323, 3) and counts == SIZES and shape == (323,)
    x, counts, shape = du._batch_layout(Cn, lat, pts, torch.tensor(SIZES))                   # a CPU int tensor
    assert counts == SIZES
    x, counts, shape = du._batch_layout(Cn, lat[:3], torch.zeros(3, 5, 3), None)
    assert x.shape == (15, 3) and counts == [5, 5, 5] and shape == (3, 5)
    for bad in (torch.zeros(len(SIZES), Cn + 1), torch.zeros(Cn), torch.zeros(1, len(SIZES), Cn)):
        with pytest.raises(ValueError, match=r'\(S, C\) = \(S, 8\)'):
            du._batch_layout(Cn, bad, pts, SIZES)
    with pytest.raises(ValueError, match='counts sum to 324, but there are 323 points'):
        du._batch_layout(Cn, lat, pts, [2] + SIZES[1:])
    with pytest.raises(ValueError, match='segment sizes'):
        du._batch_layout(Cn, lat, pts, SIZES[:-1])
    with pytest.raises(ValueError, match='segment sizes'):
        du._batch_layout(Cn, lat, pts, [-1, 66] + SIZES[2:])
    with pytest.raises(ValueError, match=r'\(S, N, 3\)'):
        du._batch_layout(Cn, lat, pts, None)                      # a flat list without counts
    with pytest.raises(ValueError, match='flat list'):
        du._batch_layout(Cn, lat[:3], torch.zeros(3, 5, 3), [5, 5, 5])
    # CPU tensors raise as decode_sdf does; a code in every input row stays unsupported
    for fn in (du.decode_sdf_batch, du.decode_sdf_gradient_batch):
        with pytest.raises(RuntimeError, match='must be on the GPU'):
            fn(None, lat, pts, counts=SIZES)
        with pytest.raises(NotImplementedError):
            fn(None, None, pts, counts=SIZES)
    with pytest.raises(RuntimeError, match='must be on the GPU'):
        du.decode_sdf(None, lat[:1], pts)
