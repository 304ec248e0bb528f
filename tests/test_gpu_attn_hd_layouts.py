"""Exact arithmetic for the bf16 chunk-streaming kernels at head_dim 32, 96 and 128 (csrc/attn_hd.hip: hdim::fwd_kernel,
bwd_dq_kernel, bwd_dkv_kernel) in every layout and at every edge of their 64-key chunks.

tests/test_gpu_attn_head_dims.py holds these kernels exactly at contig L = 33, 129, 257, 385 and one SPACE shape; the float64
tests hold the other layouts to 2 TOL[bf16] only.  The three bodies own the lin_in / lin_out / attn_cls_row addressing, the
routing of a shared cls row to dqkv_cls + s ld_dqkv in both backward kernels, the barriers that idle waves still meet and the
padded-key masks, so here (cases of tests/exact_attn.py, _run_exact of test_gpu_attn_head_dims.py: out, dqkv and the
per-sequence cls rows equal RNE(exact), the lse standard, every guard untouched):
  contig       S = 3, H = 3; L = 34 (waves 1..3 of the workgroup are idle and only meet the barriers), 63, 64, 65 (one short of a
               chunk, a chunk, one past), 96, 97 (three 32-row tiles, and one past), 127, 128 (one short of two chunks, and two
               chunks = a workgroup's 128 rows), 191, 193 (one short of, and one past, three chunks);
  time_cls     L = T + 1 = 33, 64, 65, 129; two clips at L = 33, so the clip stride and the `+ b` of the token rows matter;
  space_nocls  L = P = 33, 64, 65, 129; the cls rows of qkv are NaN, those of dqkv +0;
  space        L = P + 1 = 33, 64, 65, 129: a sequence that ends on a chunk edge with the shared cls row as its key 0;
  round        the forward's RNE store, contig L = 129 and time_cls L = 65 (V in 128..255: ties and inexact values);
  determinism  one case per layout, forward and backward, bit for bit.
T != P throughout.  CASES lists every case for tests/test_exact_attn_graded_premise.py, which builds them on the CPU.
"""
import functools

import pytest
import torch

import exact_attn as A
import test_gpu_exact_attention as E
from test_gpu_attn_head_dims import HDS, _run_exact
from test_gpu_long_attention import _bits

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16

CASES = set()              # (layout, dims, H, hd, kind, bwd); dims = (S, L) or (B, T, P)


def case(layout, dims, hd, H=3, kind='exact', bwd=True):
    key = (layout, tuple(dims), H, hd, kind, bwd)
    CASES.add(key)
    return key


@functools.lru_cache(maxsize=None)
def build(key):
    layout, dims, H, hd, kind, bwd = key
    make = {'contig': A.contig_case, 'space': A.space_case, 'time_cls': A.time_cls_case, 'space_nocls': A.space_nocls_case}[layout]
    return make(*dims, H, kind, bwd, hd=hd)


def _id(key):
    layout, dims, H, hd, kind, bwd = key
    return f'{layout}-{"x".join(map(str, dims))}-hd{hd}'


CONTIG = [case('contig', (3, L), hd) for hd in HDS for L in (34, 63, 64, 65, 96, 97, 127, 128, 191, 193)]
LAYOUTS = [case(layout, dims, hd) for hd in HDS for layout, shapes in (
    ('time_cls', ((2, 32, 3), (1, 63, 2), (1, 64, 2), (1, 128, 2))),
    ('space_nocls', ((2, 3, 33), (2, 2, 64), (1, 2, 65), (1, 2, 129))),
    ('space', ((2, 3, 32), (2, 2, 63), (1, 2, 64), (1, 2, 128)))) for dims in shapes]
ROUND = [case(layout, dims, hd, kind='round', bwd=False) for hd in HDS for layout, dims in (('contig', (3, 129)), ('time_cls', (1, 64, 2)))]
TWICE = [case('contig', (3, 193), 96), case('time_cls', (1, 128, 2), 32), case('space_nocls', (1, 2, 129), 128), case('space', (2, 2, 63), 96)]


@pytest.mark.parametrize('key', CONTIG, ids=_id)
def test_contig_exact_at_chunk_edges(key):
    _run_exact(build(key))


@pytest.mark.parametrize('key', LAYOUTS, ids=_id)
def test_layouts_exact(key):
    _run_exact(build(key))


@pytest.mark.parametrize('key', ROUND, ids=_id)
def test_forward_round_exact(key):
    c = build(key)
    assert c.hd in HDS and c.L > 32
    E.run_fwd(c, BF16)


@pytest.mark.parametrize('key', TWICE, ids=_id)
def test_is_bit_reproducible(key):
    c = build(key)
    first, again = _run_exact(c), _run_exact(c)
    for a, b in zip(first, again):
        if a is not None:
            assert torch.equal(_bits(a), _bits(b)), 'second run differs'
