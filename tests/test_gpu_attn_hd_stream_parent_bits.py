"""The chunk-streaming attention kernels at head_dim 32, 96 and 128 against a build of the parent commit, bit for bit: fp32 is
csrc/attn_hd_f32.hip, the bodies of csrc/attn_stream.h over F32Tiles<HD, CHUNK>; bf16 is csrc/attn_hd.hip, whose three kernel
bodies are its own and whose tile helpers are Bf16Tiles<HD, 64> (the shared bodies over Bf16Tiles at these head dims are not
compiled into the library, so the bf16 rows do not cover them).  The summation order of every product is fixed, so whatever a
build computes here it has to compute the same as the build before it: out, lse, dqkv and the per-sequence cls rows are compared as
whole buffers, the NaN sentinels of tests/exact.py around them included (8 pad columns per row, two rows after the last, the
tail of lse) -- the guarded-buffer launcher of tests/test_gpu_attn_head_dims.py.  The head_dim-64 routes of the same bodies are
held to the parent by test_long_is_the_parent_bit_for_bit, test_f32_mfma_is_the_parent_bit_for_bit,
test_head_dim_64_is_the_parent_bit_for_bit and test_fp32_head_dim_64_is_the_parent_bit_for_bit.

H = 2 and the smallest shapes at which each edge exists:
  contig (S = 2)   L = 33: one key past a 32-row tile; 65: one past a 64-row chunk; 129: a second row block with three idle
                   waves; 257; fp32 at 96 and 128, where the kernels of one call differ in their chunk rows, also 63, 64, 97
  space            (B, T, P) = (2, 3, 40) and (1, 2, 130): the cls row, more than one row block
  time_cls         (1, 40, 3)
  space_nocls      (2, 3, 33)
The parent library (VTX_PARENT_LIB, the child-process mechanism of tests/test_gpu_long_attention.py; skipped when the variable
names no file) computes all rows in ONE child process (a process start costs more than the kernels).
"""
import pytest
import torch

from helpers import report
from test_gpu_attn_head_dims import HDS, _geometry, _launch
from test_gpu_kernels import rnd
from test_gpu_long_attention import _bits, parent_build_cases

pytestmark = pytest.mark.gpu
H = 2
CONTIG = [33, 65, 129, 257]
CONTIG_CHUNK_EDGES = [63, 64, 97]                                       # fp32 at head_dim 96 and 128
LAYOUTS = [('space', (2, 3, 40)), ('space', (1, 2, 130)), ('time_cls', (1, 40, 3)), ('space_nocls', (2, 3, 33))]
ROWS = [(dtype, hd) for dtype in ('bfloat16', 'float32') for hd in HDS]
NAMES = ('out', 'lse', 'dqkv', 'dqkv_cls')


def _shapes(dtype, hd):
    lengths = CONTIG + (CONTIG_CHUNK_EDGES if dtype == 'float32' and hd in (96, 128) else [])
    return [('contig', (2, L)) for L in sorted(lengths)] + LAYOUTS


def hd_stream_cases(rows):
    """{'dtype hd': {case: [out, lse, dqkv(, dqkv_cls)] as allocated, on the CPU}} of this process's library at its defaults."""
    import vtx
    vtx.set_option('attn_hd', 'mfma')
    vtx.set_option('attn_f32', 'mfma')
    res = {}
    for name, hd in rows:
        dtype, row = getattr(torch, name), {}
        for layout, dims in _shapes(name, hd):
            S, L, B, T, P, nrows, orows, rin, rout, grp = _geometry(layout, dims)
            assert L > 32                                               # csrc/attn.hip: attn_route
            qkv, do = rnd(nrows, 3 * H * hd, seed=L + hd) * 1.5, rnd(orows, H * hd, seed=L + hd + 1)
            got = _launch(layout, tuple(dims), H, hd, dtype, qkv, do)
            row[f'{layout} {" ".join(str(d) for d in dims)}'] = [t.cpu() for t in got if t is not None]
        res[f'{name} {hd}'] = row
    return res


@pytest.fixture(scope='module')
def parent(tmp_path_factory):
    """(what the parent build computes for every row, its file name)"""
    return parent_build_cases(hd_stream_cases, [list(r) for r in ROWS], tmp_path_factory.mktemp('attn_hd_stream_parent'))


@pytest.mark.parametrize('dtype,hd', ROWS, ids=[f'{"bf16" if d == "bfloat16" else "fp32"}-{hd}' for d, hd in ROWS])
def test_streaming_kernels_are_the_parent_bit_for_bit(dtype, hd, parent):
    want, lib = parent
    row = f'{dtype} {hd}'
    got = hd_stream_cases([[dtype, hd]])[row]
    shapes = _shapes(dtype, hd)
    assert sorted(got) == sorted(want[row]) and len(got) == len(shapes) == (11 if dtype == 'float32' and hd != 32 else 8)
    for (layout, _), case in zip(shapes, got):
        assert case.startswith(layout)
        assert len(got[case]) == len(want[row][case]) == (4 if layout in ('space', 'time_cls') else 3)
        for name, a, b in zip(NAMES, got[case], want[row][case]):
            assert a.dtype == b.dtype and a.shape == b.shape
            assert torch.isfinite(a.float()).any(), f'{row}, {case}: {name} was never written'
            assert torch.equal(_bits(a), _bits(b)), \
                f'{row}, {case}: {name} differs from the parent in {int((_bits(a) != _bits(b)).sum())} of {a.numel()} elements'
    line = f'ok   streaming attention {dtype} head_dim {hd} bit-identical to {lib} on {len(got)} shapes (whole buffers): ' + ', '.join(got)
    print(line)
    report(line)
