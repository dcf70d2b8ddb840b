"""Host-side checks of the compacted backward tile's generated loops (csrc/gen_dense_asm.py::gen_compact(NOB, 'zero')): no GPU needed.
(The transposed k-major pack DecoderDev::Wkb has no read-back from Python -- like Wk -- so its layout is covered on the device only, by the
byte comparisons of tests/test_gpu_compact_bwd.py.)"""
import importlib.util
import os
import re

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'dist-renderer_amd', 'csrc')


@pytest.fixture(scope='module')
def gen():
    spec = importlib.util.spec_from_file_location('gen_dense_asm', os.path.join(CSRC, 'gen_dense_asm.py'))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _instructions(text):
    return re.findall(r'^\s+"(.*?)\\n"$', text, flags=re.M)


@pytest.mark.parametrize('nob', [4, 2])
def test_zero_form_is_the_bias_form_without_the_bias(gen, nob):
    """Same stream as the forward's loop -- every load, MFMA and loop instruction in the same order -- except that the bias tuples are
    never read and the first MFMA of every accumulator takes the constant 0 as srcC."""
    name_b, text_b = gen.gen_compact(nob, 'bias')
    name_z, text_z = gen.gen_compact(nob, 'zero')
    assert (name_b, name_z) == ('dense_asm_compact_n%d_bias' % nob, 'dense_asm_compact_n%d_zero' % nob)
    ib, iz = _instructions(text_b), _instructions(text_z)
    assert not any('%[bias]' in x for x in iz) and 'biasaddr' not in text_z
    firsts = [x for x in iz if x.startswith('v_mfma') and x.endswith(', 0')]
    assert len(firsts) == 2 * nob                                   # one per accumulator tile (row block x sample block)
    assert sorted(x.split()[1] for x in firsts) == sorted('%%[c%d%d],' % (ob, rb) for ob in range(nob) for rb in range(2))
    # without bias reads, waits and srcC operands the two forms are the same instruction for instruction
    def core(ins):
        out = []
        for x in ins:
            if '%[bias]' in x or x.startswith('s_waitcnt lgkmcnt'):
                continue
            out.append(re.sub(r', (a\[\d+:\d+\]|0)$', ', C0', x) if x.startswith('v_mfma') else x)
        return out
    assert core(ib) == core(iz)
    # an accumulator never appears as srcC before its first, zero-started MFMA
    seen = set()
    for x in iz:
        if x.startswith('v_mfma'):
            dst, srcc = x.split()[1].rstrip(','), x.split()[-1]
            assert srcc == ('0' if dst not in seen else dst), x
            seen.add(dst)


def test_header_holds_the_zero_forms():
    hdr = open(os.path.join(CSRC, 'distr_dense_asm.hpp')).read()
    for name in ('dense_asm_compact_n4_bias', 'dense_asm_compact_n2_bias', 'dense_asm_compact_n4_zero', 'dense_asm_compact_n2_zero'):
        assert len(re.findall(r'void %s\(' % name, hdr)) == 1, name
