"""Exact-arithmetic parity of vtx_attn_fwd / vtx_attn_bwd in the two layouts of the space-then-time operator order,
VTX_ATTN_TIME_CLS and VTX_ATTN_SPACE_NOCLS, in every kernel family that serves them, and of `probs` in every strided layout.

Cases are tests/exact_attn.py's routed scores (time_cls_case, space_nocls_case, space_case); runners and standards are
those of tests/test_gpu_exact_attention.py, test_gpu_long_attention.py and test_gpu_f32_attention.py:
  bf16 MFMA kernels (packed, one-workgroup, fused, dq + dkv pairs, chunk-streaming)
                           every output equals RNE(exact value): out, dqkv, the per-sequence cls rows;
  VALU and exact-fp32 kernels   out equals the exact value (RNE for bf16); dqkv and the cls rows inside the
                           (8 + n) 2^-24 sum|terms| interval of exact_attn.value_bounds;
  lse                      exactly 0 for one winner, within 4 fp32 ulps of k ln 2 otherwise;
  probs                    zeros exact, 2^-k within 2 fp32 ulps.
qkv has 8 NaN pad columns (ld_qkv = 3D + 8) and, for SPACE_NOCLS, NaN cls rows; outputs have 8 sentinel pad columns,
sentinel rows after the last sequence and a sentinel tail on lse and probs.  TIME_CLS: dqkv_cls has one row per sequence
(b, p) and is compared before vtx_cls_qkv_reduce folds the P rows of a clip, so a row scattered to the neighbouring
sequence shows although the folded sum is right.  SPACE_NOCLS: dqkv_cls is NULL and the cls rows of dqkv hold +0 over
exactly 3D columns.

Every clip count is >= 2 where the route allows, so the clip stride 1 + P T and the `+ b` of the TIME_CLS token rows
matter; T != P throughout; head_dim 64.  The docstring of each test names the kernels (attn.hip: attn_route,
attn_mfma.hip: the launchers) it reaches.  CASES lists every case for tests/test_exact_attn_premise.py, which builds them
on the CPU.
"""
import pytest
import torch

import test_gpu_exact_attention as E

pytestmark = pytest.mark.gpu
BF16, F32 = torch.bfloat16, torch.float32

CASES = set()              # (layout, B, T, P, H, kind, bwd) of every case below
BENCH_CASES = set()        # the cases with more items than persistent workgroups (built by the premise file's bench-scale test)


def case(layout, B, T, P, H=3, kind='exact', bwd=True, bench=False):
    key = (layout, B, T, P, H, kind, bwd)
    (BENCH_CASES if bench else CASES).add(key)
    return key


def build(key):
    layout, B, T, P, H, kind, bwd = key
    return {'space': E.space, 'time_cls': E.time_cls, 'space_nocls': E.space_nocls}[layout](B, T, P, H, kind, bwd)


def tc(B, T, P, H=3, **kw):
    return case('time_cls', B, T, P, H, **kw)


def nc(B, T, P, H=3, **kw):
    return case('space_nocls', B, T, P, H, **kw)


@pytest.fixture
def attn_long():
    """set(value) -> vtx.set_option('attn_long', value); back to the default afterwards (vtx_opts does not know it)."""
    import vtx
    try:
        yield lambda v: vtx.set_option('attn_long', v)
    finally:
        vtx.set_option('attn_long', '1')


@pytest.fixture
def attn_f32():
    """set(value) -> vtx.set_option('attn_f32', value); back to the default afterwards (vtx_opts does not know it)."""
    import vtx
    try:
        yield lambda v: vtx.set_option('attn_f32', v)
    finally:
        vtx.set_option('attn_f32', 'mfma')


def run(key, dtype, exact, probs=False):
    """Forward (+ backward of a backward case).  exact: RNE equality of the gradients (bf16 MFMA kernels) or the interval
    check (VALU and fp32 kernels); out is compared for equality either way."""
    c = build(key)
    qkv, out, lse = E.run_fwd(c, dtype, probs)
    res = (out, lse)
    if c.bwd:
        res += E.run_bwd(c, dtype, qkv, out, lse, exact)
    return res


def _bits(t):
    return t.view(torch.int16) if t.dtype == BF16 else t.view(torch.int32)


def _same_bits(first, again):
    for a, b in zip(first, again):
        if a is not None:
            assert torch.equal(_bits(a), _bits(b)), 'second run differs'


# ------------------------------------------------------------------------------------------------ bf16, TIME_CLS
TC_SMALL = [tc(3, 2, 7, 5), tc(3, 4, 7, 5), tc(3, 31, 4, 5)]


@pytest.mark.parametrize('hw', ['0', '3', '16'])
@pytest.mark.parametrize('key', TC_SMALL, ids=['L3', 'L5', 'L32'])
def test_time_cls_packed_exact(key, hw, vtx_opts):
    """attn_fwd_small_kernel<HW, true> / attn_bwd_small_kernel<HW, true>, HW = false (attn_hw = 0) and true (3, 16 heads per
    workgroup; H = 5 divides into neither).  L = 3 and 5: 10 and 6 sequences per 32-row tile, S = 21 a multiple of neither,
    tiles straddle clips; L = 32: one sequence fills the tile."""
    vtx_opts('attn_hw_fwd', hw)
    vtx_opts('attn_hw_bwd', hw)
    run(key, BF16, True)


TC_MFMA0 = [tc(2, 32, 3), tc(2, 96, 2)]


@pytest.mark.parametrize('fused', ['default', '0'])
@pytest.mark.parametrize('key', TC_MFMA0, ids=['L33', 'L97'])
def test_time_cls_mfma_exact(key, fused, vtx_opts):
    """attn_fwd_mfma_kernel<0>; backward attn_bwd_fused_mfma_kernel<0> (default) or, with attn_fused=0, the pair
    attn_bwd_dq_mfma_kernel<0> + attn_bwd_dkv_mfma_kernel<0, 0>.  L = 33: one key past a tile; 97: three tiles + 1."""
    if fused != 'default':
        vtx_opts('attn_fused', fused)
    run(key, BF16, True)


TC_MANY = tc(2, 32, 49, 3)


def test_time_cls_fused_several_items_exact():
    """attn_bwd_fused_mfma_kernel<0> with S H = 294 items on 256 persistent workgroups: some take a second item, whose
    group codes are drawn independently of the first one's.  A second run is bit-identical."""
    _same_bits(run(TC_MANY, BF16, True), run(TC_MANY, BF16, True))


TC_197 = tc(1, 196, 2)
TC_257 = tc(1, 256, 2)


def test_time_cls_7_tiles_exact():
    """L = 197 in a layout that is not mg_mode: attn_fwd_mfma_kernel<7> + attn_bwd_fused_mfma_kernel<7> (T = 196 frames:
    beyond any shipped model, accepted by the ABI)."""
    run(TC_197, BF16, True)


def test_time_cls_long_exact():
    """L = 257: attn_fwd_long_kernel, attn_bwd_dq_long_kernel, attn_bwd_dkv_long_kernel (chunk-streaming, bf16 policy)."""
    run(TC_257, BF16, True)


TC_VALU = [tc(3, 8, 7), tc(2, 96, 2)]


@pytest.mark.parametrize('key', TC_VALU, ids=['L9', 'L97'])
def test_time_cls_valu_bf16_exact(key, vtx_opts):
    """attn_valu=1: attn_fwd_kernel / attn_bwd_dq_kernel / attn_bwd_dkv_kernel<bf16>.  L = 9 packs G = 14 sequences per
    workgroup (S = 21); L = 97 is one sequence per workgroup with a ragged 64-key tile.  Gradients: the interval check."""
    vtx_opts('attn_valu', '1')
    run(key, BF16, False)


# ------------------------------------------------------------------------------------------------ bf16, SPACE_NOCLS
NC_TILE = [nc(3, 4, 1), nc(3, 4, 5), nc(3, 4, 16), nc(2, 3, 32)]


@pytest.mark.parametrize('key', NC_TILE, ids=['P1', 'P5', 'P16', 'P32'])
def test_space_nocls_one_tile_exact(key):
    """attn_fwd_mfma_kernel<0> + attn_bwd_fused_mfma_kernel<0> at a single 32-row tile, the branch only this layout enters:
    32 - P zero-filled pad rows that must be masked, rows T apart from lin_in's row0 = base."""
    run(key, BF16, True)


NC_TILES = [nc(2, 3, 33), nc(2, 8, 49), nc(2, 3, 256)]


@pytest.mark.parametrize('key', NC_TILES, ids=['P33', 'P49', 'P256'])
def test_space_nocls_several_tiles_exact(key):
    """attn_fwd_mfma_kernel<0>; backward attn_bwd_fused_mfma_kernel<0> (P = 33, 49) and, at 8 tiles (P = 256), the pair
    attn_bwd_dq_mfma_kernel<0> + attn_bwd_dkv_mfma_kernel<0, 0>."""
    run(key, BF16, True)


NC_196 = nc(2, 3, 196)


def test_space_nocls_196_exact():
    """The 224^2 / 16 shape at default options: attn_fwd_mfma_kernel<7> + attn_bwd_fused_mfma_kernel<7> (not mg_mode)."""
    run(NC_196, BF16, True)


@pytest.mark.parametrize('dkv', ['0', '1', '2', '3', '4'])
def test_space_nocls_196_pair_exact(dkv, vtx_opts):
    """attn_fused=0: attn_bwd_dq_mfma_kernel<7> + attn_bwd_dkv_mfma_kernel<NTK, VAR>; attn_dkv = 0..4 selects <0, 0>,
    <7, 1>, <7, 0>, <7, 2>, <7, 3> (launch_t<7, 0, 0>, <7, 7, 1>, <7, 7, 0>, <7, 7, 2>, <7, 7, 3>)."""
    vtx_opts('attn_fused', '0')
    vtx_opts('attn_dkv', dkv)
    run(NC_196, BF16, True)


NC_MANY = nc(6, 8, 196, 12, bench=True)


def test_space_nocls_196_several_items_exact():
    """attn_bwd_fused_mfma_kernel<7> with S H = 576 items on 256 persistent workgroups (forward attn_fwd_mfma_kernel<7>, one
    workgroup per item).  A second run is bit-identical."""
    _same_bits(run(NC_MANY, BF16, True), run(NC_MANY, BF16, True))


NC_LONG = [nc(2, 2, 257, 2), nc(1, 2, 784, 2)]


@pytest.mark.parametrize('key', NC_LONG, ids=['P257', 'P784'])
def test_space_nocls_long_exact(key):
    """attn_fwd_long_kernel, attn_bwd_dq_long_kernel, attn_bwd_dkv_long_kernel: one key past two chunk pairs; the 448^2 / 16
    shape."""
    run(key, BF16, True)


NC_300 = nc(2, 3, 300, 2)


def test_space_nocls_long_0_valu_exact(attn_long):
    """attn_long=0 above 256 tokens: the VALU kernels <bf16>, one sequence per workgroup.  Gradients: the interval check."""
    attn_long('0')
    run(NC_300, BF16, False)


NC_VALU = [nc(3, 4, 16), NC_196]


@pytest.mark.parametrize('key', NC_VALU, ids=['P16', 'P196'])
def test_space_nocls_valu_bf16_exact(key, vtx_opts):
    """attn_valu=1: the VALU kernels <bf16>.  P = 16 packs G = 8 sequences per workgroup, S = 12 not a multiple of 8;
    P = 196 is one sequence per workgroup."""
    vtx_opts('attn_valu', '1')
    run(key, BF16, False)


# ------------------------------------------------------------------------------------------------ fp32
F32_CASES = {
    'time_cls L9 valu-packed': (tc(3, 8, 7), 'mfma'),
    'time_cls L33': (tc(2, 32, 3), 'mfma'),
    'time_cls L97': (tc(2, 96, 2), 'mfma'),
    'time_cls L97 attn_f32=valu': (tc(2, 96, 2), 'valu'),
    'space_nocls P16 valu-packed': (nc(3, 4, 16), 'mfma'),
    'space_nocls P49': (nc(2, 8, 49), 'mfma'),
    'space_nocls P196': (NC_196, 'mfma'),
    'space_nocls P784': (nc(1, 2, 784, 2), 'mfma'),
    'space_nocls P196 attn_f32=valu': (NC_196, 'valu'),
}


@pytest.mark.parametrize('name', list(F32_CASES))
def test_f32_layouts_exact(name, attn_f32):
    """Up to 32 tokens: the VALU kernels <float>, packed.  Above, attn_f32=mfma: attn_fwd_f32_kernel, attn_bwd_dq_f32_kernel,
    attn_bwd_dkv_f32_kernel (chunk-streaming, fp32 policy); attn_f32=valu: the VALU kernels <float>.  out equals the exact
    value, gradients inside exact_attn.value_bounds."""
    key, opt = F32_CASES[name]
    attn_f32(opt)
    run(key, F32, False)


# ------------------------------------------------------------------------------------------------ probs
PROBS = {
    'space P8': case('space', 2, 3, 8, 2),
    'space P196': case('space', 2, 3, 196, 2),
    'time_cls L9': tc(3, 8, 7),
    'time_cls L33': tc(2, 32, 3),
    'space_nocls P16': nc(3, 4, 16),
    'space_nocls P196': NC_196,
}


@pytest.mark.parametrize('dtype', [F32, BF16], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('name', list(PROBS))
def test_probs_layouts_exact(name, dtype, attn_f32):
    """probs= : attn_fwd_kernel<T, 64, 1> after the forward of the route (bf16: VALU at space P = 8, packed at time_cls
    L = 9, the MFMA kernels otherwise; fp32: the VALU forward), rows gathered through in_row.  out, lse and probs are checked
    and the probs tail is untouched.  fp32 above 32 tokens: attn_route sends a probs request to the VALU forward and not to
    attn_fwd_f32_kernel -- out and lse are bit-identical to the forward with attn_f32=valu."""
    c = build(PROBS[name])
    _, out, lse = E.run_fwd(c, dtype, probs=True)
    if dtype == F32 and c.L > 32:
        attn_f32('valu')
        _, out_v, lse_v = E.run_fwd(c, dtype)
        assert torch.equal(_bits(out), _bits(out_v)) and torch.equal(_bits(lse), _bits(lse_v)), \
            'a probs request did not take the VALU forward'


# ------------------------------------------------------------------------------------------------ forward, round
R = dict(kind='round', bwd=False)
ROUND = {
    'time_cls small<true, true>': (tc(3, 10, 7, 5, **R), {}),
    'time_cls small<false, true>': (tc(3, 10, 7, 5, **R), {'attn_hw_fwd': '0'}),
    'time_cls mfma<0> L33': (tc(2, 32, 3, **R), {}),
    'space_nocls one tile P16': (nc(3, 4, 16, **R), {}),
    'space_nocls mfma<7> P196': (nc(2, 3, 196, **R), {}),
    'space_nocls long P300': (nc(2, 3, 300, 2, **R), {}),
    'space_nocls valu P16': (nc(3, 4, 16, **R), {'attn_valu': '1'}),
}


@pytest.mark.parametrize('family', list(ROUND))
def test_forward_round_layouts_exact(family, vtx_opts):
    """V in 128..255: a share of the outputs are exact ties and most are inexact, so RNE at the O store of every family
    shows on the two layouts: attn_fwd_small_kernel<true, true> and <false, true> (L = 11: two sequences per tile, S = 21
    odd; at L = 9 only 39.1 % of the outputs are inexact, below the 40 % the round premise asks), attn_fwd_mfma_kernel<0>
    (two tiles and one), attn_fwd_mfma_kernel<7>, attn_fwd_long_kernel, attn_fwd_kernel<bf16> packed."""
    key, opts = ROUND[family]
    for k, v in opts.items():
        vtx_opts(k, v)
    run(key, BF16, True)
