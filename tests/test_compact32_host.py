"""Host-side checks of the compacted 32-ray tile's generated loops (csrc/gen_dense_asm.py::gen_compact(NOB, 'bias', RB=1)): no GPU needed.
The RB = 1 loop is the RB = 2 loop with the second ray block's reads and MFMAs removed and X rows of 128 bytes instead of 256."""
import importlib.util
import os
import re
import subprocess
import sys

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


def _b_reg(gen, x):
    """(buffer, k-step, ray block) of the B register a ds_read_b32 / v_mfma names."""
    v = int(re.search(r'ds_read_b32 v(\d+),', x).group(1)) if x.startswith('ds_read_b32') else int(x.split(', ')[2][1:])
    buf = 0 if v < gen.B[1] else 1
    return buf, (v - gen.B[buf]) // 2, (v - gen.B[buf]) % 2


def _halve_rows(gen, x):
    """A B read of the 64-ray loop (ray block 0) at the same row of a 32-ray X: every row is half as long."""
    m = re.match(r'(ds_read_b32 v\d+, \S+) offset:(\d+)$', x)
    assert m and int(m.group(2)) % 256 == 0, x         # (ray block 0 reads the start of a 256-byte row)
    return '%s offset:%d' % (m.group(1), int(m.group(2)) // 2)


@pytest.mark.parametrize('nob', [4, 2])
def test_rb1_is_rb2_without_the_second_ray_block(gen, nob):
    name2, text2 = gen.gen_compact(nob, 'bias', 2)
    name1, text1 = gen.gen_compact(nob, 'bias', 1)
    assert (name2, name1) == ('dense_asm_compact_n%d_bias' % nob, 'dense_asm_compact_n%d_r1_bias' % nob)
    assert gen.gen_compact(nob, 'bias') == (name2, text2)               # (RB defaults to the 64-ray tile)
    assert 'f32x16 (&acc)[%d][1]' % nob in text1 and 'f32x16 (&acc)[%d][2]' % nob in text2
    i2, i1 = _instructions(text2), _instructions(text1)
    # the 32-ray loop never names a register, an accumulator or a column of the second ray block
    for x in i1:
        if x.startswith('v_mfma') or x.startswith('ds_read_b32'):
            assert _b_reg(gen, x)[2] == 0, x
        assert not re.search(r'%\[c\d1\]', x), x
    assert not re.search(r'\[c\d1\]', text1)
    # MFMAs: the same sequence once ray block 1's are struck out (same A register, same B register of block 0, same accumulator, same srcC)
    m2 = [x for x in i2 if x.startswith('v_mfma') and _b_reg(gen, x)[2] == 0]
    m1 = [x for x in i1 if x.startswith('v_mfma')]
    assert m1 == m2 and 2 * len(m1) == len([x for x in i2 if x.startswith('v_mfma')])
    # B reads: ray block 0's, in the same order, at rows of 128 bytes
    r2 = [_halve_rows(gen, x) for x in i2 if x.startswith('ds_read_b32') and _b_reg(gen, x)[2] == 0]
    r1 = [x for x in i1 if x.startswith('ds_read_b32')]
    assert r1 == r2 and 2 * len(r1) == len([x for x in i2 if x.startswith('ds_read_b32')])
    # the running X address advances by whole groups of eight 128-byte rows
    adds2 = [x for x in i2 if x.startswith('v_add_u32 v%d' % gen.VX)]
    adds1 = [x for x in i1 if x.startswith('v_add_u32 v%d' % gen.VX)]
    assert [int(x.split(', ')[1]) for x in adds2] == [2 * int(x.split(', ')[1]) for x in adds1] == [8 * 256, 16 * 256]
    # everything else -- weight gathers, index reads, bias tuples, the loop's scalar instructions -- is the same stream in the same order
    def rest(ins):
        return [x for x in ins if not (x.startswith('v_mfma') or x.startswith('ds_read_b32') or x.startswith('s_waitcnt lgkmcnt') or x.startswith('v_add_u32 v%d' % gen.VX))]
    assert rest(i1) == rest(i2)
    # from the loop's label on (the prologue's partial waits are the generator's own queue model): an MFMA reads an A / B register only
    # behind a full wait that follows the register's load -- also where a gap holds two loads (NOB = 2: 8 MFMAs, 12 loads per group)
    pending, in_loop = set(), False
    for x in i1:
        if x.startswith('.Ldense_compact_loop'):
            in_loop = True
        elif x.startswith('ds_read_b32') or x.startswith('buffer_load'):
            lo = int(re.search(r' v\[?(\d+)', x).group(1))
            n = {'ds_read_b32': 1, 'buffer_load_dwordx4': 4, 'buffer_load_dwordx2': 2}[x.split()[0]]
            pending |= set(range(lo, lo + n))
        elif x == 's_waitcnt vmcnt(0) lgkmcnt(0)':
            pending.clear()
        elif x.startswith('v_mfma') and in_loop:
            a, b = (int(t[1:]) for t in x.split(', ')[1:3])
            assert a not in pending and b not in pending, x


def test_generator_output_is_the_committed_header():
    out = subprocess.run([sys.executable, os.path.join(CSRC, 'gen_dense_asm.py')], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    with open(os.path.join(CSRC, 'distr_dense_asm.hpp')) as f:
        assert out.stdout == f.read(), 'distr_dense_asm.hpp is not what gen_dense_asm.py writes: regenerate it'


def test_header_holds_the_rb1_forms_and_the_dispatcher_picks_them():
    hdr = open(os.path.join(CSRC, 'distr_dense_asm.hpp')).read()
    for name in ('dense_asm_compact_n4_r1_bias', 'dense_asm_compact_n2_r1_bias'):
        assert len(re.findall(r'void %s\(' % name, hdr)) == 1, name
    for nob in (4, 2):
        assert 'constexpr (NOB == %d && BIAS && RB == 1) dense_asm_compact_n%d_r1_bias(' % (nob, nob) in hdr
        assert 'constexpr (NOB == %d && BIAS && RB == 2) dense_asm_compact_n%d_bias(' % (nob, nob) in hdr
        assert 'constexpr (NOB == %d && !BIAS && RB == 2) dense_asm_compact_n%d_zero(' % (nob, nob) in hdr
    assert 'RB == 1) dense_asm_compact_n4_r1_zero' not in hdr           # (the backward has no 32-sample compacted tile)
