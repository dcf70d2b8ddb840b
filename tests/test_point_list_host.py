"""Host-side pins of the point-list plumbing (no GPU): the public workspace sizes, which are ABI (callers allocate by them), and how
the two engine classes are constructed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import PKG


def _constant(header, name):
    with open(os.path.join(PKG, 'csrc', header)) as f:
        return int(re.search(r'constexpr int %s = (\d+);' % name, f.read()).group(1))


@pytest.mark.parametrize('n', [0, 1, 31, 32, 33, 64, 65, 4097])
def test_plain_workspace_sizes(n):
    """distr_mlp_workspace_bytes = the latent constants + alignment slack; the backward adds one partial per 32 points + slack."""
    from distr import binding
    L = binding.lib()
    HID, PSTRIDE = _constant('distr_mlp.hpp', 'HID'), _constant('distr_kernels.hpp', 'PSTRIDE')
    fwd = 2 * HID * 4 + 256
    assert L.distr_mlp_workspace_bytes(n) == fwd
    assert L.distr_mlp_backward_workspace_bytes(n) == fwd + (n + 31) // 32 * PSTRIDE * 4 + 256


def test_segmented_workspace_sizes():
    """The literals are what the commit before the plain and the segmented list shared one carve returned for these counts:
    3 x 4096 B of constants + the 768 B tile table + 256, and for the backward 3 tiles x 4160 B rounded up to 256 on top."""
    from distr import binding
    L = binding.lib()
    cnt = (C.c_int64 * 3)(65, 0, 1)
    assert L.distr_mlp_multi_workspace_bytes(3, cnt) == 13312
    assert L.distr_mlp_backward_multi_workspace_bytes(3, cnt) == 25856


class _Ctx(object):
    """Stands in for binding.Context (which needs a device): records the uploads."""

    def __init__(self, device_index=0):
        self.uploads = []

    def set_decoder(self, flat, nlat):
        self.uploads.append(('sdf', len(flat), nlat))

    def set_color_decoder(self, flat, nlat):
        self.uploads.append(('color', len(flat), nlat))


def test_engine_construction(monkeypatch, fixture_decoder):
    """From raw weights or from a module: every engine has counted its upload and knows its code length; a refresh counts again."""
    import torch
    from core.graph.deep_sdf_decoder import Decoder
    from distr import binding, functions
    monkeypatch.setattr(binding, 'Context', _Ctx)
    Ws, bs, _ = fixture_decoder
    raw = functions.engine_from_weights(Ws, bs, 0)
    assert isinstance(raw, functions.DecoderEngine) and raw.generation == 1 and raw.latent_size == 256
    dec = Decoder(256, [512] * 8, norm_layers=(), latent_in=[4]).eval()
    built = functions.get_engine(dec, 0)
    assert built.generation == 1 and built.latent_size == 256 and functions.get_engine(dec, 0) is built and built.generation == 1
    with torch.no_grad():
        dec.lin0.bias.add_(1.0)                         # an in-place edit: the next get_engine uploads again
    assert functions.get_engine(dec, 0).generation == 2
    assert [u[0] for u in raw.ctx.uploads + built.ctx.uploads] == ['sdf'] * 3
    rs = np.random.RandomState(0)
    cs = 8
    OUT = [512, 512, 512, 253, 512, 512, 512, 512, 3]
    IN = [256 + cs + 3, 512, 512, 512, 253 + 256 + cs + 3, 512, 512, 512, 512]
    color = functions.ColorEngine(weights=([rs.rand(o, i).astype(np.float32) for o, i in zip(OUT, IN)], [rs.rand(o).astype(np.float32) for o in OUT]))
    assert color.generation == 1 and color.latent_size == 256 + cs and color.ctx.uploads[0][0] == 'color'
