"""The bf16 MFMA attention kernels for 33..256 tokens (csrc/attn_mfma.hip) against a build of the parent commit, bit for bit,
on ordinary random data: out, lse, dqkv and the per-frame cls rows of every instantiation the options reach.  The kernels of
that file are schedules around one set of tile bodies (fwd_query_tile, score_pair, dq_ds / dq_accumulate, dkv_probs /
dkv_accumulate, row_delta, the destination rows, the LDS-DMA request); tests/test_gpu_exact_attention.py holds each of them to
exact arithmetic, here the whole output equals what the library named by VTX_PARENT_LIB computes (the child-process mechanism
of tests/test_gpu_long_attention.py; skipped when the variable names no file).

  defaults             fwd <0>, one-pass <0> (33, 130 tokens: ragged; 256: dq / dk,dv <0, 0>, eight full tiles), the streamed
                       forward / backward (197; 224 = seven full tiles); 30 x 12 = 360 and 5 x 8 x 12 = 480 items: more than
                       one item per persistent workgroup on 256 CUs; the cls row of the space layout (36 and 196 patches)
  attn_fwd_stream=0    fwd <7>
  attn_fused=1         one-pass <0> and <7>; 360 items for its persistent loop
  attn_fused=0         dq <7> with dk,dv <7, 0 | 7, VAR> under attn_dkv = 0 .. 4; dq / dk,dv <0> at 37 and 256 tokens and with
                       a cls row
The parent library computes all rows in ONE child process (a process start costs more than the kernels).
"""
import pytest
import torch

from helpers import report
from test_gpu_long_attention import _bits, parent_build_cases, parent_cases

pytestmark = pytest.mark.gpu

ROWS = {
    'defaults': dict(options={}, contig=[(3, 33, 3), (3, 130, 3), (3, 197, 3), (3, 224, 3), (3, 256, 3), (30, 197, 12)],
                     space=[(5, 8, 196, 12), (2, 3, 36, 2)]),
    'attn_fwd_stream=0': dict(options={'attn_fwd_stream': '0'}, contig=[(3, 197, 3)], space=[(2, 3, 196, 2)]),
    'attn_fused=1': dict(options={'attn_fused': '1'}, contig=[(3, 33, 3), (3, 197, 3), (30, 65, 12)], space=[]),
    **{f'attn_fused=0 attn_dkv={v}': dict(options={'attn_fused': '0', 'attn_dkv': str(v)}, contig=[(4, 197, 3)], space=[])
       for v in range(5)},
    'attn_fused=0': dict(options={'attn_fused': '0'}, contig=[(4, 37, 3), (4, 256, 3)], space=[(2, 3, 36, 2)]),
}
DEFAULTS = {'attn_fwd_stream': '1', 'attn_fused': '2', 'attn_dkv': '3'}          # tests/conftest.py: _OPTION_DEFAULTS


def _spec(row):
    # every row names all three switches: the rows run one after another in one process
    return dict(dtype='bfloat16', options={**DEFAULTS, **ROWS[row]['options']}, contig=[list(c) for c in ROWS[row]['contig']],
                space=[list(c) for c in ROWS[row]['space']])


def attn_mfma_cases(rows):
    """{row: {case: [out, lse, dqkv(, dqkv_cls)] on the CPU}} of this process's library."""
    return {row: parent_cases(_spec(row)) for row in rows}


@pytest.fixture(scope='module')
def parent(tmp_path_factory):
    """(what the parent build computes for every row, its file name)"""
    return parent_build_cases(attn_mfma_cases, list(ROWS), tmp_path_factory.mktemp('attn_mfma_parent'))


@pytest.mark.parametrize('row', list(ROWS))
def test_attn_mfma_is_the_parent_bit_for_bit(row, parent, vtx_opts):
    want, lib = parent
    spec = _spec(row)
    for k in spec['options']:
        vtx_opts(k, DEFAULTS[k])                                 # parent_cases sets them; put back whatever happens
    got = parent_cases(spec)
    assert sorted(got) == sorted(want[row]) and len(got) == len(spec['contig']) + len(spec['space']) > 0
    for case in got:
        assert len(got[case]) == len(want[row][case]) == (4 if case.startswith('space') else 3)
        for name, a, b in zip(('out', 'lse', 'dqkv', 'dqkv_cls'), got[case], want[row][case]):
            assert a.dtype == b.dtype and a.shape == b.shape
            assert torch.isfinite(a.float()).any(), f'{row}, {case}: {name} was never written'
            assert torch.equal(_bits(a), _bits(b)), \
                f'{row}, {case}: {name} differs from the parent in {int((_bits(a) != _bits(b)).sum())} of {a.numel()} elements'
    line = f'ok   attn_mfma.hip [{row}] bit-identical to {lib} on {len(got)} shapes: ' + ', '.join(got)
    print(line)
    report(line)
