"""The exact-fp32 MFMA attention kernels at head_dim 32, 96 and 128 (csrc/attn_hd_f32.hip: fwd_kernel, bwd_dq_kernel,
bwd_dkv_kernel over HD): fp32 inputs, more than 32 tokens, all four layouts; option attn_f32 = mfma (default) | valu.  A
workgroup owns 128 queries (keys in the dk / dv kernel), a wave a 32-row tile; chunks hold 64 rows at head_dim 32, 32 rows
in the forward at 96 and 128 and in dq at 96, 64 rows in dk / dv at 96 and in dq and dk / dv at 128.

  1. exact arithmetic (tests/exact_attn.py, runners of tests/test_gpu_exact_attention.py) by the standard of
     tests/test_gpu_f32_attention.py::run_f32: out equals the exact value bit for bit, lse exactly 0 for one winner and within
     4 fp32 ulps of k ln 2 otherwise; dq, dk, dv and the per-sequence cls rows inside exact_attn.value_bounds; the sentinel
     guards untouched.  L = 33: one key past a 32-row tile (and a 32-row chunk); 65: one past a 64-row chunk (two 32-row
     chunks); 129: one past a workgroup's 128 rows; 197; 257: two blocks + 1; at 96 and 128, where kernels of one call differ
     in their chunks, also 63, 64 and 97: one short of two 32-row chunks (of one 64-row chunk), exactly that, three + 1 (one + 33);
  2. a second forward + backward is bit-identical;
  3. the switch is live: attn_f32=valu is attn_valu=1 bit for bit, attn_f32=mfma agrees with it within the bars of
     test_f32_contig_vs_float64_and_valu_at_joint_scale and differs from it somewhere;
  4. `probs`: out and lse with a probs buffer are the bits of attn_f32=valu without one, the probabilities meet probs_ok;
  5. nothing else moves: fp32 head_dim 64 and bf16 head_dim 96 against a build of the parent commit (VTX_PARENT_LIB; skipped
     otherwise); fp32 of 8 tokens at 32 / 96 / 128 and bf16 head_dim 96 bit-identical under both values of attn_f32.
"""
import functools

import pytest
import torch

import exact_attn as A
import test_gpu_exact_attention as E
from helpers import check
from test_gpu_attn_head_dims import HDS, _plain
from test_gpu_f32_attention import LSE_BAR, attn_f32  # noqa: F401  (attn_f32: fixture)
from test_gpu_kernels import TOL, dev, rnd
from test_gpu_long_attention import _bits, assert_parent_bit_for_bit, parent_build_cases

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
BF16, F32 = torch.bfloat16, torch.float32


# ------------------------------------------------------------------------------------------------ 1. exact arithmetic
@functools.lru_cache(maxsize=None)
def _contig(L, hd):
    return A.contig_case(2, L, 2, hd=hd)


@functools.lru_cache(maxsize=None)
def _layout(name, hd):
    return {'space-40': lambda: A.space_case(2, 3, 40, 2, hd=hd),
            'space-130': lambda: A.space_case(1, 2, 130, 2, hd=hd),
            'time_cls-40': lambda: A.time_cls_case(1, 40, 3, 2, hd=hd),
            'space_nocls-33': lambda: A.space_nocls_case(2, 3, 33, 2, hd=hd)}[name]()


def run_f32(c):
    """tests/test_gpu_f32_attention.py::run_f32 at these head dims"""
    assert c.hd in HDS and c.L > 32                                     # attn.hip: attn_route
    qkv, out, lse = E.run_fwd(c, F32)
    return (out, lse) + E.run_bwd(c, F32, qkv, out, lse, False)         # exact=False: the interval of fp32 probabilities


@pytest.mark.parametrize('hd', HDS)
@pytest.mark.parametrize('L', [33, 65, 129, 197, 257])
def test_contig_exact(L, hd, attn_f32):
    attn_f32('mfma')
    run_f32(_contig(L, hd))


@pytest.mark.parametrize('hd', [96, 128])
@pytest.mark.parametrize('L', [63, 64, 97])
def test_contig_exact_at_chunk_edges(L, hd, attn_f32):
    attn_f32('mfma')
    run_f32(_contig(L, hd))


@pytest.mark.parametrize('hd', HDS)
@pytest.mark.parametrize('name', ['space-40', 'space-130', 'time_cls-40', 'space_nocls-33'])
def test_layouts_exact(name, hd, attn_f32):
    attn_f32('mfma')
    run_f32(_layout(name, hd))


# ------------------------------------------------------------------------------------------------ 2. determinism
@pytest.mark.parametrize('hd', HDS)
def test_is_bit_reproducible(hd, attn_f32):
    attn_f32('mfma')
    for c in (_contig(257, hd), _layout('space-130', hd)):
        first, again = run_f32(c), run_f32(c)
        for a, b in zip(first, again):
            if a is not None:
                assert torch.equal(_bits(a), _bits(b)), 'second run differs'


# ------------------------------------------------------------------------------------------------ 3. the switch
def _operands(S, L, H, hd, dtype):
    return dev(rnd(S, L, 3 * H * hd, seed=5) * 1.5, dtype), dev(rnd(S, L, H * hd, seed=6), dtype)


@pytest.mark.parametrize('hd', HDS)
@pytest.mark.parametrize('L', [33, 197])
def test_switch_is_live(L, hd, attn_f32, vtx_opts):
    S, H = 2, 3
    qkv, do = _operands(S, L, H, hd, F32)
    attn_f32('mfma')
    new = _plain(S, L, H, hd, F32, qkv, do)
    attn_f32('valu')
    old = _plain(S, L, H, hd, F32, qkv, do)
    attn_f32('mfma')
    vtx_opts('attn_valu', '1')
    valu = _plain(S, L, H, hd, F32, qkv, do)
    assert all(torch.isfinite(t).all() for t in new)
    for a, b in zip(old, valu):
        assert torch.equal(_bits(a), _bits(b)), f'hd={hd} L={L}: attn_f32=valu differs from attn_valu=1'
    for what, a, b, bar in zip(('out', 'lse', 'dqkv'), new, old, (TOL[F32], LSE_BAR, 2 * TOL[F32])):
        check(f'attn f32 hd={hd} mfma vs valu {what} L={L}', a.cpu(), b.cpu(), bar)
    differ = sum(int((_bits(a) != _bits(b)).sum()) for a, b in zip(new, old))
    print(f'hd={hd} L={L}: {differ} elements of out / lse / dqkv differ between attn_f32=mfma and attn_f32=valu')
    assert differ > 0, f'hd={hd} L={L}: attn_f32=mfma and attn_f32=valu return the same bits: the same kernel ran'


# ------------------------------------------------------------------------------------------------ 4. probs
@pytest.mark.parametrize('hd', HDS)
def test_probs_keeps_the_valu_forward(hd, attn_f32):
    c = A.contig_case(2, 40, 2, hd=hd, seed=5)
    attn_f32('mfma')
    _, out, lse = E.run_fwd(c, F32, probs=True)                         # checks the probabilities: exact_attn.probs_ok
    attn_f32('valu')
    _, out_v, lse_v = E.run_fwd(c, F32)
    assert torch.equal(_bits(out), _bits(out_v)), f'hd={hd}: out with a probs buffer is not the VALU forward\'s'
    assert torch.equal(_bits(lse), _bits(lse_v)), f'hd={hd}: lse with a probs buffer is not the VALU forward\'s'


# ------------------------------------------------------------------------------------------------ 5. nothing else moves
def test_fp32_head_dim_64_is_the_parent_bit_for_bit(attn_f32, tmp_path):
    spec = dict(dtype='float32', options={'attn_f32': 'mfma'}, contig=[(2, 33, 3), (2, 197, 3)], space=[(2, 2, 196, 3)])
    try:
        assert_parent_bit_for_bit(spec, tmp_path, 'fp32 head_dim 64 attn_f32=mfma')
    finally:
        attn_f32('mfma')


def hd_cases(spec):
    """{case: [out, lse, dqkv]} on the CPU, contig; spec = [[dtype name, S, L, H, hd]]."""
    res = {}
    for name, S, L, H, hd in spec:
        dtype = getattr(torch, name)
        qkv, do = _operands(S, L, H, hd, dtype)
        res[f'{name} {S} {L} {H} {hd}'] = [t.cpu() for t in _plain(S, L, H, hd, dtype, qkv, do)]
    return res


def test_bf16_head_dim_96_is_the_parent_bit_for_bit(tmp_path):
    spec = [['bfloat16', 2, 197, 3, 96]]
    want, parent = parent_build_cases(hd_cases, spec, tmp_path)
    got = hd_cases(spec)
    assert sorted(got) == sorted(want) and len(got) == 1
    for case in got:
        for name, a, b in zip(('out', 'lse', 'dqkv'), got[case], want[case]):
            assert a.dtype == b.dtype and a.shape == b.shape
            assert torch.isfinite(a.float()).all(), f'{case}: {name} holds elements that were never written'
            assert torch.equal(_bits(a), _bits(b)), f'{case}: {name} differs from {parent}'


@pytest.mark.parametrize('dtype,L,hd', [(F32, 8, 32), (F32, 8, 96), (F32, 8, 128), (BF16, 197, 96)],
                         ids=['fp32-L8-32', 'fp32-L8-96', 'fp32-L8-128', 'bf16-L197-96'])
def test_other_routes_ignore_attn_f32(dtype, L, hd, attn_f32):
    S, H = 5, 3
    qkv, do = _operands(S, L, H, hd, dtype)
    attn_f32('mfma')
    new = _plain(S, L, H, hd, dtype, qkv, do)
    attn_f32('valu')
    old = _plain(S, L, H, hd, dtype, qkv, do)
    for a, b in zip(new, old):
        assert torch.isfinite(a.float()).all() and torch.equal(_bits(a), _bits(b)), f'{dtype} L={L} hd={hd}: attn_f32 changes the result'
