"""CPU-only checks of the block enumeration of the setup kernels (include/distr_live_order.h, csrc/distr_kernels.hpp block_pixel): a workgroup of
256 threads covers a 16 x 16 pixel block, each of its wavefronts one 8 x 8 sub-block. A numpy restatement against the library's host helper
(the same function the kernels call)."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

GRIDS = [(1, 1), (7, 9), (16, 16), (17, 16), (137, 137), (512, 40)]      # (w, h)


@pytest.fixture(scope='module')
def libdistr():
    from distr import binding
    binding.build_library()
    return binding.lib()


def restated(w, h):
    """[blocks][256] pixel index y * w + x of every thread, -1 outside the grid."""
    bx, by = (w + 15) // 16, (h + 15) // 16
    block, thread = np.meshgrid(np.arange(bx * by), np.arange(256), indexing='ij')
    wave, lane = thread // 64, thread % 64
    x = (block % bx) * 16 + (wave % 2) * 8 + lane % 8
    y = (block // bx) * 16 + (wave // 2) * 8 + lane // 8
    return np.where((x < w) & (y < h), y * w + x, -1)


def library(L, w, h):
    n = L.distr_block_grid(w, h)
    return np.array([[L.distr_block_pixel(w, h, b, t) for t in range(256)] for b in range(n)], dtype=np.int64).reshape(n, 256)


@pytest.mark.parametrize('w,h', GRIDS)
def test_block_enumeration(libdistr, w, h):
    got, want = library(libdistr, w, h), restated(w, h)
    assert got.shape == want.shape == (((w + 15) // 16) * ((h + 15) // 16), 256)
    assert (got == want).all()
    # a bijection onto the pixels: every pixel exactly once, everything else "no ray"
    inside = got[got >= 0]
    assert inside.size == w * h and (np.sort(inside) == np.arange(w * h)).all()
    assert (got >= -1).all() and (got < w * h).all()
    # positions outside the image map to "no ray", positions inside never do
    assert int((got < 0).sum()) == got.size - w * h
    # every wavefront (64 consecutive threads) holds one 8 x 8 sub-block: its pixels lie within 8 columns and 8 rows, all in one aligned cell
    for blk in got:
        for wave in blk.reshape(4, 64):
            px = wave[wave >= 0]
            if px.size:
                assert len(set(px % w // 8)) == 1 and len(set(px // w // 8)) == 1
    # ... and inside it the order is row-major: ascending pixel indices
    for wave in got.reshape(-1, 64):
        px = wave[wave >= 0]
        assert (np.diff(px) > 0).all()


def test_out_of_range_arguments(libdistr):
    L = libdistr
    assert L.distr_block_grid(0, 5) == 0 and L.distr_block_grid(5, 0) == 0 and L.distr_block_grid(-3, 4) == 0
    assert L.distr_block_grid(16, 16) == 1 and L.distr_block_grid(17, 16) == 2 and L.distr_block_grid(512, 40) == 32 * 3
    for block, thread in ((-1, 0), (1, 0), (0, -1), (0, 256)):
        assert L.distr_block_pixel(16, 16, block, thread) == -1


def test_header_and_binding_agree(libdistr):
    from distr import binding
    hdr = open(os.path.join(ROOT, 'include', 'distr_live_order.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    assert set(re.findall(r'\b(distr_[a-z0-9_]+)\s*\(', hdr)) == set(binding.LIVE_ORDER_EXPORTS)
    assert '#include "distr_live_order.h"' in open(os.path.join(ROOT, 'include', 'distr.h')).read()
    assert 'distr_live_order.h' in binding.HEADERS
    for name in binding.LIVE_ORDER_EXPORTS:
        assert hasattr(libdistr, name), name


def test_knobs_are_checked_at_create(libdistr):
    """DISTR_LIVE_ORDER / DISTR_RAY_BLOCKS: 0 or 1, read once at distr_create; anything else is refused with a message."""
    import ctypes as C
    from distr import binding
    for knob in ('DISTR_LIVE_ORDER', 'DISTR_RAY_BLOCKS'):
        old = os.environ.get(knob)
        try:
            os.environ[knob] = '2'
            h = C.c_void_p()
            assert libdistr.distr_create_abi(C.byref(h), 0, binding.ABI_VERSION) == -1          # DISTR_ERR_INVALID_ARG
            assert knob.encode() in libdistr.distr_last_error(h)
            libdistr.distr_destroy(h)
        finally:
            if old is None:
                del os.environ[knob]
            else:
                os.environ[knob] = old
