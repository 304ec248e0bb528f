"""Packed MFMA attention for up to 32 tokens (csrc/attn_hd.hip, attn_fwd_small_kernel / attn_bwd_small_kernel<HD, HW, CLS>: bf16,
layouts CONTIG and TIME_CLS), here at head_dim 32, 96 and 128, where option attn_hd = mfma, the default, selects it.  G = 32 / L
sequences share a 32-row tile, one wave per (tile, head).

  1. exact arithmetic (tests/exact_attn.py, runners of tests/test_gpu_exact_attention.py): every output equals RNE(exact),
     the lse meets its standard, guards and pad columns stay untouched; with one head and four tiles per workgroup
     (attn_hw_* = 0) and with 3 and 16 heads of a tile per workgroup;
  2. float64 at D = 768 (24 x 32, 8 x 96, 6 x 128: more heads than a workgroup's head group at 32, an odd group at 96 and 128
     with the default attn_hw_bwd = 4), the bars of tests/test_gpu_attn_head_dims.py;
  3. `probs`: the VALU probabilities pass behind the new forward;
  4. a second run is bit-identical;
  5. the switch is live: attn_hd=valu is attn_valu=1 bit for bit, the default route is within the bars of
     test_mfma_matches_valu of it and differs from it somewhere; fp32 and head_dim 64 ignore the switch;
  6. against a build of the parent commit, bit for bit (VTX_PARENT_LIB; skipped otherwise): all four head dims of the packed
     route on whole guarded buffers, and the two head_dim-64 tests from before the kernels were written once.
"""
import functools

import pytest
import torch

import exact_attn as A
import test_gpu_exact_attention as E
from helpers import check, report
from test_gpu_attn_head_dims import HDS, _against_f64, _geometry, _launch, _plain, attn_hd  # noqa: F401  (attn_hd: fixture)
from test_gpu_kernels import dev, rnd
from test_gpu_long_attention import _bits, assert_parent_bit_for_bit, parent_build_cases

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
BF16, F32 = torch.bfloat16, torch.float32


# ------------------------------------------------------------------------------------------------ 1. exact arithmetic
@functools.lru_cache(maxsize=None)
def _contig(S, L, H, hd, seed=0):
    c = A.contig_case(S, L, H, seed=seed, hd=hd)
    assert (c.layout, c.S, c.L, c.H, c.hd) == ('contig', S, L, H, hd)
    return c


@functools.lru_cache(maxsize=None)
def _time_cls(B, T, P, H, hd):
    c = A.time_cls_case(B, T, P, H, hd=hd)
    assert (c.layout, c.S, c.L, c.H, c.hd) == ('time_cls', B * P, T + 1, H, hd)
    return c


def _run_exact(c):
    assert c.hd in HDS and c.L <= 32
    qkv, out, lse = E.run_fwd(c, BF16)
    return (out, lse) + E.run_bwd(c, BF16, qkv, out, lse, True)


# S = 7: the last tile is partial for every L; G = 32 / L runs 6, 4, 3, 2, 1, 1; 17 is one key past half a tile
@pytest.mark.parametrize('hd', HDS)
@pytest.mark.parametrize('L', [5, 8, 9, 16, 17, 32])
def test_contig_exact(L, hd):
    _run_exact(_contig(7, L, 2, hd))


@pytest.mark.parametrize('hd', HDS)
@pytest.mark.parametrize('S,L', [(40, 1), (4, 8)], ids=['L1-two-tiles', 'L8-one-full-tile'])
def test_contig_tile_edges_exact(S, L, hd):
    """L = 1: 32 sequences a tile, 40 of them = one full tile and a quarter; L = 8, S = 4: exactly one full tile."""
    assert S * L == 32 if L == 8 else 32 < S * L < 64
    _run_exact(_contig(S, L, 2, hd))


# (2, 8, 5): L = 9; (2, 4, 9): L = 5, six sequences a tile, 9 a clip: a tile spans two clips; (1, 31, 3): L = 32;
# (3, 1, 4): L = 2, 16 sequences a tile over clips of 4: a tile across three clips
@pytest.mark.parametrize('hd', HDS)
@pytest.mark.parametrize('B,T,P', [(2, 8, 5), (2, 4, 9), (1, 31, 3), (3, 1, 4)])
def test_time_cls_exact(B, T, P, hd):
    G = 32 // (T + 1)
    if (B, T, P) == (2, 4, 9):
        assert G == 6 and P % G and G < P < 2 * G                       # the second tile starts in clip 0 and ends in clip 1
    if (B, T, P) == (3, 1, 4):
        assert G == 16 and B * P < G and G > 2 * P                      # one tile holds all three clips
    _run_exact(_time_cls(B, T, P, 2, hd))


@pytest.mark.parametrize('hw', ['0', '3', '16'])
@pytest.mark.parametrize('hd', HDS)
@pytest.mark.parametrize('layout', ['contig-L8', 'time_cls-L9'])
def test_heads_per_workgroup_exact(layout, hd, hw, vtx_opts):
    """attn_hw_* = 0: one head and four row tiles per workgroup; 3 and 16 (capped at H and at 8 waves): heads of
    one tile.  H = 5 divides into no group of 3; S = 37 / B P = 14 leave the last workgroup and tile partial."""
    vtx_opts('attn_hw_fwd', hw)
    vtx_opts('attn_hw_bwd', hw)
    _run_exact(_contig(37, 8, 5, hd) if layout == 'contig-L8' else _time_cls(2, 8, 7, 5, hd))


# ------------------------------------------------------------------------------------------------ 2. float64
@pytest.mark.parametrize('H,hd', [(24, 32), (8, 96), (6, 128)], ids=['24x32', '8x96', '6x128'])
def test_contig_against_float64_at_768(H, hd):
    _against_f64('contig', (7, 8), H, hd, BF16)


# ------------------------------------------------------------------------------------------------ 3. probs
@pytest.mark.parametrize('hd', HDS)
def test_probs_behind_the_packed_forward(hd):
    E.run_fwd(_contig(3, 9, 2, hd, seed=5), BF16, probs=True)


# ------------------------------------------------------------------------------------------------ 4. determinism
@pytest.mark.parametrize('hd', HDS)
def test_is_bit_reproducible(hd):
    for c in (_contig(7, 9, 2, hd), _time_cls(2, 8, 5, 2, hd)):
        first, again = _run_exact(c), _run_exact(c)
        for a, b in zip(first, again):
            if a is not None:
                assert torch.equal(_bits(a), _bits(b)), 'second run differs'


# ------------------------------------------------------------------------------------------------ 5. the switch
def _operands(S, L, H, hd, dtype):
    return dev(rnd(S, L, 3 * H * hd, seed=5) * 1.5, dtype), dev(rnd(S, L, H * hd, seed=6), dtype)


@pytest.mark.parametrize('hd', HDS)
def test_switch_is_live(hd, attn_hd, vtx_opts):
    S, L, H = 40, 8, 3
    qkv, do = _operands(S, L, H, hd, BF16)
    new = _plain(S, L, H, hd, BF16, qkv, do)
    attn_hd('valu')
    old = _plain(S, L, H, hd, BF16, qkv, do)
    attn_hd('mfma')
    vtx_opts('attn_valu', '1')
    valu = _plain(S, L, H, hd, BF16, qkv, do)
    assert all(torch.isfinite(t.float()).all() for t in new)
    for a, b in zip(old, valu):
        assert torch.equal(_bits(a), _bits(b)), f'hd={hd}: attn_hd=valu differs from attn_valu=1'
    for what, a, b, bar in zip(('out', 'lse', 'dqkv'), new, old, (1e-2, 1e-4, 2e-2)):
        check(f'attn hd={hd} packed mfma vs valu {what} L={L}', a.float().cpu(), b.float().cpu(), bar)
    differ = sum(int((_bits(a) != _bits(b)).sum()) for a, b in zip(new, old))
    print(f'hd={hd}: {differ} elements of out / lse / dqkv differ between attn_hd=mfma and attn_hd=valu')
    assert differ > 0, f'hd={hd}: attn_hd=mfma and attn_hd=valu return the same bits: the same kernel ran'


@pytest.mark.parametrize('dtype,hd', [(F32, 32), (F32, 96), (F32, 128), (BF16, 64)], ids=['fp32-32', 'fp32-96', 'fp32-128', 'bf16-64'])
def test_switch_leaves_fp32_and_head_dim_64_alone(dtype, hd, attn_hd):
    S, L, H = 40, 8, 3
    qkv, do = _operands(S, L, H, hd, dtype)
    attn_hd('mfma')
    new = _plain(S, L, H, hd, dtype, qkv, do)
    attn_hd('valu')
    old = _plain(S, L, H, hd, dtype, qkv, do)
    for a, b in zip(new, old):
        assert torch.isfinite(a.float()).all() and torch.equal(_bits(a), _bits(b)), f'{dtype} hd={hd}: attn_hd changes the result'


# ------------------------------------------------------------------------------------------------ 6. parent bits
def time_cls_cases(spec):
    """{case: [out, lse, dqkv, dqkv_cls]} on the CPU for head_dim 64, bf16, VTX_ATTN_TIME_CLS; spec = [[B, T, P, H]]."""
    from vtx import ops
    from vtx._lib import ATTN_TIME_CLS
    res = {}
    for B, T, P, H in spec:
        S, L, D = B * P, T + 1, H * 64
        qkv = dev(rnd(B, 1 + P * T, 3 * D, seed=1) * 1.5, BF16)
        do = dev(rnd(B * P * T + S, D, seed=2), BF16)
        o = torch.full((B * P * T + S, D), float('nan'), dtype=BF16, device=DEV)
        lse = torch.full((S * H * L,), float('nan'), device=DEV)
        ops.attn_fwd(qkv, o, lse, ATTN_TIME_CLS, S, L, H, 64, 0.125, B, T, P)
        dqkv = torch.zeros(B, 1 + P * T, 3 * D, dtype=BF16, device=DEV)     # (the clips' cls rows are written by cls_qkv_reduce, not here)
        dcls = torch.full((S, 3 * D), float('nan'), dtype=BF16, device=DEV)
        ops.attn_bwd(qkv, o, lse, do, dqkv, ATTN_TIME_CLS, S, L, H, 64, 0.125, B, T, P, dqkv_cls=dcls)
        torch.cuda.synchronize()
        res[f'time_cls {B} {T} {P} {H}'] = [t.cpu() for t in (o, lse, dqkv, dcls)]
    return res


PACKED_HDS = (32, 64, 96, 128)
PACKED_DEFAULT = [('contig', (40, 1)), ('contig', (7, 8)), ('contig', (7, 9)), ('contig', (7, 17)), ('contig', (7, 32)),
                  ('time_cls', (2, 8, 5)), ('time_cls', (2, 4, 9))]                  # H = 2; (2, 4, 9): a tile spans two clips
# attn_hw_fwd = attn_hw_bwd = hw: H = 5, where 3 divides no group; H = 12, where the cap of 16 waves at head_dim 64 and of 8
# elsewhere differ (hw = 16: one group of 12 heads against groups of 8 and 4)
PACKED_HW = [(hw, dims, H) for hw in ('0', '3', '16') for dims, H in (((37, 8), 5), ((5, 8), 12))]


def packed_cases(hds):
    """{'hd': {case: [out, lse, dqkv(, dqkv_cls)] as allocated, on the CPU}} of this process's library: the packed route, bf16,
    guarded buffers (the launcher of tests/test_gpu_attn_head_dims.py)."""
    import vtx
    vtx.set_option('attn_hd', 'mfma')
    res = {}
    try:
        for hd in hds:
            row = {}
            for hw, layout, dims, H in [('', lay, d, 2) for lay, d in PACKED_DEFAULT] + [(hw, 'contig', d, H) for hw, d, H in PACKED_HW]:
                for opt, default in (('attn_hw_fwd', '16'), ('attn_hw_bwd', '4')):
                    vtx.set_option(opt, hw or default)
                S, L, B, T, P, nrows, orows, rin, rout, grp = _geometry(layout, dims)
                assert L <= 32                                          # csrc/attn.hip: attn_route
                qkv, do = rnd(nrows, 3 * H * hd, seed=L + hd) * 1.5, rnd(orows, H * hd, seed=L + hd + 1)
                got = _launch(layout, tuple(dims), H, hd, BF16, qkv, do)
                row[f'{layout} {" ".join(str(d) for d in dims)} H={H}' + (f' hw={hw}' if hw else '')] = [t.cpu() for t in got if t is not None]
            res[str(hd)] = row
    finally:
        vtx.set_option('attn_hw_fwd', '16')
        vtx.set_option('attn_hw_bwd', '4')
    return res


def test_packed_route_is_the_parent_bit_for_bit(tmp_path):
    """Every head dim of the packed kernels against a build of the parent commit (where head_dim 64 was a copy of its own in
    csrc/attn_mfma.hip): whole guarded buffers, NaN sentinels included; all rows in one child process."""
    want, lib = parent_build_cases(packed_cases, list(PACKED_HDS), tmp_path)
    got = packed_cases(PACKED_HDS)
    assert sorted(got) == sorted(want) == sorted(str(hd) for hd in PACKED_HDS)
    for hd in got:
        assert sorted(got[hd]) == sorted(want[hd]) and len(got[hd]) == len(PACKED_DEFAULT) + len(PACKED_HW) == 13
        for case in got[hd]:
            assert len(got[hd][case]) == len(want[hd][case]) == (4 if case.startswith('time_cls') else 3)
            for name, a, b in zip(('out', 'lse', 'dqkv', 'dqkv_cls'), got[hd][case], want[hd][case]):
                assert a.dtype == b.dtype and a.shape == b.shape
                assert torch.isfinite(a.float()).any(), f'head_dim {hd}, {case}: {name} was never written'
                assert torch.equal(_bits(a), _bits(b)), \
                    f'head_dim {hd}, {case}: {name} differs from the parent in {int((_bits(a) != _bits(b)).sum())} of {a.numel()} elements'
        line = f'ok   packed attention bfloat16 head_dim {hd} bit-identical to {lib} on {len(got[hd])} shapes (whole buffers): ' + ', '.join(got[hd])
        print(line)
        report(line)


def test_head_dim_64_contig_is_the_parent_bit_for_bit(tmp_path):
    spec = dict(dtype='bfloat16', options={}, contig=[[5, 8, 3], [5, 9, 3]], space=[])
    assert_parent_bit_for_bit(spec, tmp_path, 'head_dim 64 packed')


def test_head_dim_64_time_cls_is_the_parent_bit_for_bit(tmp_path):
    spec = [[2, 8, 5, 3]]
    want, parent = parent_build_cases(time_cls_cases, spec, tmp_path)
    got = time_cls_cases(spec)
    assert sorted(got) == sorted(want) and len(got) == 1
    for case in got:
        for name, a, b in zip(('out', 'lse', 'dqkv', 'dqkv_cls'), got[case], want[case]):
            assert a.dtype == b.dtype and a.shape == b.shape
            assert torch.isfinite(a.float()).all(), f'{case}: {name} holds elements that were never written'
            assert torch.equal(_bits(a), _bits(b)), f'{case}: {name} differs from {parent}'
