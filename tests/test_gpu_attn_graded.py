"""Graded exact cases on every multi-block attention forward: the rescale of the online softmax at factors other than 0 and 1.

The routed cases of tests/exact_attn.py give every winner the raw score 0, so in the four restatements of the chunked forward
(fwd_query_tile of csrc/attn_mfma.hip, the forward body of csrc/attn_stream.h, hdim::fwd_kernel of csrc/attn_hd.hip, the
forward of csrc/xattn_mfma.hip)
    alpha = exp2((m - mn) c2),  l = l alpha + bl,  acc *= alpha,  e = exp2(fma(s, c2, -mn c2))
alpha is 1 where the running maximum stays and 0 where a chunk of losers is wiped: a factor of the wrong magnitude passes.
The 'graded' kind (exact_attn.py) makes c2 exactly 2^-3 and grades the winners' scores in steps of 8, so that in every
(sequence, head) item at least 8 queries per chunk boundary carry a maximum across it that is lower by 8 or 16 than the one
they find behind it: alpha is 1/2 or 1/4 there, every probability a power of two, and the final maximum is 0, -8 or -16.

  bf16 kernels   out equals the exact value; lse within 4 fp32 ulps at |k ln 2| plus 2 at |top ln 2| of (k - top) ln 2;
  fp32 kernels   (attn_f32.hip, attn_hd_f32.hip: the attn_stream.h body, P stays fp32) out inside exact_attn.value_bounds,
                 the same lse standard; how many outputs equal the exact value goes to the parity report, unasserted.
Buffers are guarded as in tests/test_gpu_exact_attention.py, whose runners these are; a second run is bit-identical.  Shapes are
the smallest that cross a block of the kernel.  CASES lists every case for tests/test_exact_attn_graded_premise.py, which builds
them on the CPU and shows that emulated faults of the rescale fail them.
"""
import functools

import pytest
import torch

import exact_attn as A
import test_gpu_exact_attention as E
from test_gpu_f32_attention import attn_f32  # noqa: F401  (fixture: conftest's vtx_opts does not know the switch)

pytestmark = pytest.mark.gpu
BF16, F32 = torch.bfloat16, torch.float32
HDS = [32, 96, 128]

CASES = set()              # (layout, dims, H, hd) of every case below; dims = (S, L), (B, T, P) or (B, Lq, Lk)


def case(layout, dims, H, hd=64):
    key = (layout, tuple(dims), H, hd)
    CASES.add(key)
    return key


@functools.lru_cache(maxsize=None)
def build(key):
    layout, dims, H, hd = key
    if layout == 'cross':
        return A.cross_case(*dims, H, hd, 'graded', False)
    make = {'contig': A.contig_case, 'space': A.space_case, 'time_cls': A.time_cls_case, 'space_nocls': A.space_nocls_case}[layout]
    return make(*dims, H, 'graded', False, hd=hd)


def _bits(t):
    return t.view(torch.int16) if t.dtype == BF16 else t.view(torch.int32)


def run(key, dtype):
    """The forward twice: both runs meet the standard, and the second returns the bits of the first."""
    c = build(key)
    assert c.kind == 'graded' and c.scale == A.SCALE_GRADED
    runs = []
    for _ in range(2):
        runs.append(E.run_cross(c, dtype, True) if c.layout == 'cross' else E.run_fwd(c, dtype)[1:])
    for a, b in zip(*runs):
        assert torch.equal(_bits(a), _bits(b)), 'second run differs'


def _id(key):
    layout, dims, H, hd = key
    return f'{layout}-{"x".join(map(str, dims))}-hd{hd}'


# fwd_query_tile (attn_mfma.hip): head_dim 64, 33..256 tokens; blocks of MA_KB = 4 key tiles, so two blocks above 128 keys.
# attn_fwd_stream selects attn_fwd_stream_mfma_kernel<7> or attn_fwd_mfma_kernel<7> at 193..224 tokens (space P = 196) and
# leaves the other shapes on attn_fwd_mfma_kernel<0>.
MFMA = [case('contig', (2, 129), 3), case('contig', (2, 256), 3), case('space', (2, 2, 196), 2), case('time_cls', (2, 129, 2), 3),
        case('space_nocls', (2, 2, 130), 3)]


@pytest.mark.parametrize('stream', ['0', '1'])
@pytest.mark.parametrize('key', MFMA, ids=_id)
def test_attn_mfma_graded(key, stream, vtx_opts):
    vtx_opts('attn_fwd_stream', stream)
    run(key, BF16)


# attn_fwd_long_kernel (attn_long.hip: stream_fwd, bf16 policy, chunks of 128 keys): head_dim 64 above 256 tokens.
LONG = [case('contig', (2, 257), 3), case('contig', (2, 385), 2), case('space', (1, 2, 300), 2)]


@pytest.mark.parametrize('key', LONG, ids=_id)
def test_attn_long_graded(key):
    run(key, BF16)


# hdim::fwd_kernel (attn_hd.hip: chunks of 64 keys): bf16, head_dim 32, 96 and 128 above 32 tokens.  L = 65 in all four layouts
# (space P = 64 and time_cls T = 64 with the shared cls row as key 0), 129 and 257.
HD_SHAPES = [('contig', (2, 65), 3), ('contig', (2, 129), 2), ('contig', (2, 257), 2), ('space', (1, 2, 64), 2),
             ('time_cls', (1, 64, 3), 2), ('space_nocls', (1, 2, 65), 2)]
HD = [case(*shape, hd) for hd in HDS for shape in HD_SHAPES]


@pytest.mark.parametrize('key', HD, ids=_id)
def test_attn_hd_graded(key):
    run(key, BF16)


# fwd_kernel of xattn_mfma.hip (chunks of 128 keys, Lq != Lk): one key past a chunk; three chunks and a ragged fourth.
CROSS = [case('cross', dims, 2, hd) for hd in (64, 96) for dims in ((2, 40, 129), (1, 70, 393))]


@pytest.mark.parametrize('key', CROSS, ids=_id)
def test_xattn_graded(key):
    run(key, BF16)


# attn_fwd_f32_kernel (attn_f32.hip) and the forward of attn_hd_f32.hip: stream_fwd with the fp32 policy, chunks of 32 or 64
# keys; fp32 inputs above 32 tokens with attn_f32=mfma, the default.
FP32 = [case('contig', (2, 257), 2, 64)] + [case('contig', (2, L), 2, hd) for hd in HDS for L in (65, 129)]


@pytest.mark.parametrize('key', FP32, ids=_id)
def test_f32_graded(key, attn_f32):
    attn_f32('mfma')
    run(key, F32)
