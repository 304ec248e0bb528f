"""The VALU attention kernels of csrc/attn.hip at head_dim 32, 96 and 128: attn_fwd_kernel<T, HD, 0 / 1>, attn_bwd_dq_kernel<T, HD,
NP> (two column parts of dq above 64, picked by blockIdx.z) and attn_bwd_dkv_kernel<T, HD>, fp32 and bf16.  Six of these instances
spill to scratch (dk / dv at 96 and 128, dq at 128; profiles/attn_hd_bench.txt, 1).

Routing.  The default route is VALU for fp32 of up to 32 tokens in every layout, for bf16 SPACE and SPACE_NOCLS of up to 32 tokens and
for every `probs` pass (attn.hip: attn_route): those cases run with default options, and one case per (dtype, head dim, layout) is
also held bit for bit to a run under attn_valu=1.  Every other case runs under attn_valu=1, the first line of attn_route (attn_hd=valu
and attn_f32=valu are pinned to it bit for bit by tests/test_gpu_attn_head_dims.py and tests/test_gpu_attn_hd_f32.py).

  a. exact arithmetic, contig (tests/exact_attn.py, runners and VALU standard of tests/test_gpu_exact_attention.py): out equals the
     exact value (RNE for bf16), lse exactly 0 for one winner and within 4 fp32 ulps of k ln 2 otherwise, dq / dk / dv inside
     exact_attn.value_bounds; pad columns, trailing rows and tails untouched.  CONTIG names the edge each shape reaches;
  b. the same in SPACE, TIME_CLS and SPACE_NOCLS: the per-sequence cls rows, the untouched clip cls rows, cls_qkv_reduce, the +0 cls
     rows of SPACE_NOCLS; time_cls and space_nocls carry NaN pad columns in qkv;
  c. `round` forward cases: RNE at the O store, bf16;
  d. `probs` (attn_fwd_kernel<T, HD, 1>) with default options behind whichever forward ran;
  e. float64 on dense random data and on a ramp (tests/test_gpu_attn_head_dims.py: _against_f64 at its bars).  The routed cases never
     move the running maximum above 0 and leave half the columns of dq and dk zero; dense data fills both gaps, and the ramp moves the
     maximum at every 8-key chunk and across every 64-key tile (tests/test_attn_valu_hd_premise.py: a rescale skipped at a tile
     boundary changes about 3 % of the rows of random data at L = 65 and more than half of the ramp's);
  f. a second forward + backward is bit-identical, on shapes that reach all six spilling instances.
"""
import functools

import pytest
import torch

import exact_attn as A
import test_gpu_attn_head_dims as HDM
import test_gpu_exact_attention as E

pytestmark = pytest.mark.gpu
BF16, F32 = torch.bfloat16, torch.float32
HDS = HDM.HDS
H = 2
DTYPES = pytest.mark.parametrize('dtype', [F32, BF16], ids=['fp32', 'bf16'])

# a. (S, L): AT_PACK_THREADS = 128 threads hold G = 128 // L sequences of L <= 64 rows; above, 256 threads hold one row block of one
# sequence and the keys come in 64-key tiles
CONTIG = [(37, 1),        # G = 128; the largest LDS image (the 4-float pad counts 128 times)
          (37, 8),        # packed; S = 37 is no multiple of any G, so the last group is partial
          (37, 9),        # G = 14; two idle threads
          (37, 32),       # packed
          (37, 33),       # G = 3
          (37, 43),       # G = 2; the first L with two sequences
          (37, 64),       # G = 2; full tile; the largest L = 64 image
          (3, 65),        # G = 1; a second key tile of one key
          (3, 130),       # three key tiles
          (3, 257),       # a second row block of one row; a fifth key tile of one key
          (2, 300)]       # several key tiles; a ragged second row block
# b. (B, T, P)
LAYOUTS = {'space': [(2, 3, 8), (2, 3, 31), (2, 3, 40), (1, 2, 130), (1, 2, 256)],
           'time_cls': [(2, 8, 5), (2, 4, 9), (1, 31, 3), (1, 40, 3), (2, 96, 2), (1, 256, 2)],
           'space_nocls': [(2, 3, 5), (3, 4, 16), (2, 3, 32), (2, 3, 33), (2, 3, 64), (1, 2, 196), (1, 2, 257)]}
LAYOUT_CASES = [(layout, dims) for layout, cases in LAYOUTS.items() for dims in cases]
# c. (layout, dims, H)
ROUND = [('contig', (3, 130), 3), ('contig', (37, 8), 5), ('space', (2, 3, 8), 2)]
# d. (layout, dims, seed)
PROBS = [('contig', (3, 9), 5), ('contig', (3, 40), 5), ('contig', (2, 65), 5), ('contig', (2, 130), 5),
         ('space', (2, 3, 8), 0), ('space', (1, 2, 130), 0), ('time_cls', (2, 8, 5), 0), ('space_nocls', (3, 4, 16), 0)]
# e.
F64_CONTIG = [8, 32, 43, 64, 65, 130, 257]
F64_LAYOUTS = [('space', (2, 3, 8)), ('space', (2, 3, 40)), ('space', (1, 2, 300)), ('time_cls', (2, 8, 5)), ('time_cls', (1, 40, 3)),
               ('space_nocls', (3, 4, 16)), ('space_nocls', (2, 3, 33))]
F64_RAMP = [65, 130, 257]
# f.
TWICE = [(37, 8), (37, 64), (3, 130)]
# one default-route case per layout for the route proof
ROUTE = {'contig': (37, 8), 'space': (2, 3, 8), 'time_cls': (2, 8, 5), 'space_nocls': (2, 3, 5)}

_BUILD = {'contig': A.contig_case, 'space': A.space_case, 'time_cls': A.time_cls_case, 'space_nocls': A.space_nocls_case}


@functools.lru_cache(maxsize=None)
def build(layout, dims, hd, heads=H, kind='exact', bwd=True, seed=0):
    return _BUILD[layout](*dims, heads, kind, bwd, seed, hd=hd)


def seq_len(layout, dims):
    return {'contig': lambda: dims[1], 'space': lambda: dims[2] + 1, 'time_cls': lambda: dims[1] + 1, 'space_nocls': lambda: dims[2]}[layout]()


def default_is_valu(dtype, layout, L):
    """attn.hip: attn_route without a `probs` request at head_dim 32, 96 and 128"""
    return L <= 32 and (dtype == F32 or layout in ('space', 'space_nocls'))


def route(vtx_opts, dtype, layout, L):
    if not default_is_valu(dtype, layout, L):
        vtx_opts('attn_valu', '1')


def _same_bits(first, again, what):
    for a, b in zip(first, again):
        if a is not None:
            assert torch.equal(HDM._bits(a), HDM._bits(b)), what


# ------------------------------------------------------------------------------------------------ a. exact, contig
@DTYPES
@pytest.mark.parametrize('hd', HDS)
@pytest.mark.parametrize('S,L', CONTIG)
def test_contig_exact(S, L, hd, dtype, vtx_opts):
    route(vtx_opts, dtype, 'contig', L)
    E.run_self(build('contig', (S, L), hd), dtype, valu=True)


# ------------------------------------------------------------------------------------------------ b. exact, layouts
@DTYPES
@pytest.mark.parametrize('hd', HDS)
@pytest.mark.parametrize('layout,dims', LAYOUT_CASES)
def test_layouts_exact(layout, dims, hd, dtype, vtx_opts):
    route(vtx_opts, dtype, layout, seq_len(layout, dims))
    E.run_self(build(layout, dims, hd), dtype, valu=True)


@pytest.mark.parametrize('hd', HDS)
@pytest.mark.parametrize('dtype,layout', [(F32, 'contig'), (F32, 'space'), (F32, 'time_cls'), (F32, 'space_nocls'), (BF16, 'space'),
                                          (BF16, 'space_nocls')],
                         ids=['fp32-contig', 'fp32-space', 'fp32-time_cls', 'fp32-space_nocls', 'bf16-space', 'bf16-space_nocls'])
def test_default_route_is_the_valu_kernels(dtype, layout, hd, vtx_opts):
    """Up to 32 tokens the default options and attn_valu=1 return the same bits: the default cases above ran these kernels."""
    dims = ROUTE[layout]
    assert default_is_valu(dtype, layout, seq_len(layout, dims))
    c = build(layout, dims, hd)
    first = E.run_self(c, dtype, valu=True)
    vtx_opts('attn_valu', '1')
    _same_bits(first, E.run_self(c, dtype, valu=True), f'{layout} {dims} hd={hd}: the default route differs from attn_valu=1')


# ------------------------------------------------------------------------------------------------ c. round
@pytest.mark.parametrize('hd', HDS)
@pytest.mark.parametrize('layout,dims,heads', ROUND)
def test_forward_round_exact(layout, dims, heads, hd, vtx_opts):
    route(vtx_opts, BF16, layout, seq_len(layout, dims))
    E.run_self(build(layout, dims, hd, heads, 'round', False), BF16, valu=True)


# ------------------------------------------------------------------------------------------------ d. probs
@DTYPES
@pytest.mark.parametrize('hd', HDS)
@pytest.mark.parametrize('layout,dims,seed', PROBS)
def test_probs_exact(layout, dims, seed, hd, dtype):
    E.run_fwd(build(layout, dims, hd, seed=seed), dtype, probs=True)


# ------------------------------------------------------------------------------------------------ e. float64
@DTYPES
@pytest.mark.parametrize('hd', HDS)
@pytest.mark.parametrize('L', F64_CONTIG)
def test_contig_against_float64(L, hd, dtype, vtx_opts):
    route(vtx_opts, dtype, 'contig', L)
    HDM._against_f64('contig', (3, L), H, hd, dtype)


@DTYPES
@pytest.mark.parametrize('hd', HDS)
@pytest.mark.parametrize('layout,dims', F64_LAYOUTS)
def test_layouts_against_float64(layout, dims, hd, dtype, vtx_opts):
    route(vtx_opts, dtype, layout, seq_len(layout, dims))
    HDM._against_f64(layout, dims, H, hd, dtype)


@DTYPES
@pytest.mark.parametrize('hd', HDS)
@pytest.mark.parametrize('L', F64_RAMP)
def test_ramp_against_float64(L, hd, dtype, vtx_opts):
    route(vtx_opts, dtype, 'contig', L)
    HDM._against_f64('contig', (3, L), H, hd, dtype, 'ramp')


# ------------------------------------------------------------------------------------------------ f. determinism
@DTYPES
@pytest.mark.parametrize('hd', [96, 128])
@pytest.mark.parametrize('S,L', TWICE)
def test_is_bit_reproducible(S, L, hd, dtype, vtx_opts):
    route(vtx_opts, dtype, 'contig', L)
    c = build('contig', (S, L), hd)
    _same_bits(E.run_self(c, dtype, valu=True), E.run_self(c, dtype, valu=True), f'contig {S} x {L} hd={hd}: second run differs')
