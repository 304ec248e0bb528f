"""Register block flow of the persistent NT GEMM (csrc/gemm_nt.hip): in the continuous kernels the epilogue's residual /
multiplier block goes from HBM straight into registers behind the main loop, and the ring keeps the operand flow.

Every case is held to the exact expected values (integer operands, dyadic scales: tests/exact.py) and, bit for bit on the
whole output buffer with its guards, to the per-tile flow (`pp_cont=0`), which stages the block through LDS.

  epilogues   residual; residual with a row scale; multiplier (dgelu_kind 1, a stored bf16 factor); residual with C and R
              through the token map (the group boundary falls inside a tile and inside a 16-row pass, the cls rows keep
              their sentinel); scale_split (split rows take no residual and go to Csplit)
  K           192, 256, 320: 3, 4 and 5 K tiles (the continuous flow's minimum; the ring parity of a tile's K tile 0
              alternates with odd counts)
  N           256 and 320 (a ragged last column tile: chunks beyond N read chunk 0)
  M           600 = two full row tiles + 88 rows (rows beyond M read the last valid row); 2360 under pp_grid = 8 (several
              tiles per workgroup: the block registers of one tile must not reach the next) and pp_grid = 256
  guards      8 guard columns behind every output row, sentinel rows behind Csplit and in the cls rows; R and the
              multiplier are allocated without a spare row
  fallback    a periodic residual and a table map on R with several boundaries per tile are routed to the per-tile flow
              by the launcher: same results under both settings

The cases are built like exact.nt_epilogue_case (same generators and reference), which is fixed to M = 2364."""
import functools

import pytest
import torch

import exact as X

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
DEV = 'cuda:0'
T = 2
LAYOUT = {600: (2, 300), 2360: (4, 590)}          # M -> (clips, tokens per clip): 300 % 16 = 12, 590 % 16 = 14
EPILOGUES = ('residual', 'residual_scale', 'mul', 'residual_tok', 'scale_split', 'periodic', 'residual_tab')
FALLBACK = ('periodic', 'residual_tab')
TAB_STEP = 3                                       # table map on R: logical row m -> m + 3 * (m // tokens)


def dev(t, dtype=None):
    return (t.to(dtype) if dtype is not None else t).to(DEV).contiguous()


@functools.lru_cache(maxsize=None)
def case(epi, M, N, K):
    """CPU tensors of one launch and its float64 expected result ('round' cases: bias offset 512, every store rounds)."""
    B, ntok = LAYOUT[M]
    kind = 'round' if epi in ('residual', 'mul', 'residual_tok') else 'exact'
    seed = M + N + K
    A, W, bias = X.nt_operands(M, N, K, kind, seed)
    scales = dict(choices=(0.5, 1.0, 2.0)) if kind == 'round' else dict(choices=(0.0, 0.5, 1.0, 2.0))
    c = dict(M=M, N=N, K=K, kind=kind, A=A, W=W, bias=bias, h=None, scale=None, rs=(1, 0, 1, 0), R=None, r_period=0,
             split_row=0, tok=False, rtab=False)
    if epi == 'residual':
        R = X.ints((M, N), -32, 32, 1.0, seed + 6)
        c.update(R=R, expected=X.nt_reference(epi, A, W, bias=bias, R=R))
    elif epi == 'residual_scale':                                 # rs = (T, 1, 1, 0): s[m // T]
        R = X.ints((M, N), -32, 32, 1.0, seed + 6)
        s = X.dyadic_scales(M // T, seed + 4, **scales)
        c.update(R=R, scale=s, rs=(T, 1, 1, 0), expected=X.nt_reference(epi, A, W, bias=bias, scale=s.repeat_interleave(T), R=R))
    elif epi == 'mul':
        h = X.ints((M, N), -2, 2, 1.0, seed + 3)
        h = torch.where(h == 0, torch.ones_like(h), h)
        c.update(h=h, expected=X.nt_reference(epi, A, W, bias=bias, h=h))
    elif epi == 'residual_tok':                                   # A, C and R rows through the token map
        Xp = torch.zeros(B, 1 + ntok, K)
        Xp[:, 1:] = A.reshape(B, ntok, K)
        Xp[:, 0] = X.ints((B, K), -1, 1, 1.0, seed + 5)          # cls rows the map must skip: non-zero
        R = X.ints((B, 1 + ntok, N), -32, 32, 1.0, seed + 6)
        c.update(A=Xp, R=R, tok=True, amap_tok=True,
                 expected=X.nt_reference(epi, A, W, bias=bias, R=R[:, 1:].reshape(M, N)).reshape(B, ntok, N))
    elif epi == 'scale_split':
        # M token rows, then B*T split rows to Csplit; scale index rs = (ntok, T, T, 1): token m -> s[(m // ntok) * T + m % T],
        # split row m -> s[m - M]; residual (through the token map) on the token rows only
        Mo = M + B * T
        A2, _, _ = X.nt_operands(Mo, N, K, kind, seed + 8)
        s = X.dyadic_scales(B * T, seed + 9, **scales)
        R = X.ints((B, 1 + ntok, N), -32, 32, 1.0, seed + 6)
        m = torch.arange(M)
        tok_s = s[(m // ntok) * T + m % T]
        c.update(A=A2, M=Mo, scale=s, rs=(ntok, T, T, 1), R=R, tok=True, split_row=M,
                 expected=X.nt_reference(epi, A2[:M], W, bias=bias, scale=tok_s, R=R[:, 1:].reshape(M, N)).reshape(B, ntok, N),
                 expected_split=X.nt_reference(epi + ' split', A2[M:], W, bias=bias, scale=s))
    elif epi == 'periodic':                                       # C rows through the token map, R row m % ntok
        E = X.ints((ntok, N), -32, 32, 1.0, seed + 7)
        c.update(R=E, r_period=ntok, tok=True,
                 expected=X.nt_reference(epi, A, W, bias=bias, R=E.repeat(B, 1)).reshape(B, ntok, N))
    elif epi == 'residual_tab':                                   # R through a table map with more than one boundary per tile
        grp = 100
        R = X.ints((M + TAB_STEP * ((M - 1) // grp), N), -32, 32, 1.0, seed + 6)
        rows = torch.arange(M) + TAB_STEP * (torch.arange(M) // grp)
        c.update(R=R, rtab=grp, expected=X.nt_reference(epi, A, W, bias=bias, R=R[rows]))
    else:
        raise ValueError(epi)
    c['expected'] = X.expect_bf16(f'{epi} {M}x{N}x{K}', c['expected'], kind)
    if 'expected_split' in c:
        c['expected_split'] = X.expect_bf16(f'{epi} split {M}x{N}x{K}', c['expected_split'], kind)
    return c


@functools.lru_cache(maxsize=None)
def operands(epi, M, N, K):
    """Device copies of a case's inputs, made once and left unchanged."""
    c = case(epi, M, N, K)
    d = dict(A=dev(c['A'], BF16), W=dev(c['W'], BF16), bias=dev(c['bias']))
    for k in ('h', 'R'):
        if c[k] is not None:
            d[k] = dev(c[k], BF16)
    if c['scale'] is not None:
        d['scale'] = dev(c['scale'])
    return d


def launch(epi, M, N, K):
    """One launch under the options in force; returns (whole output buffer, compared view, guards, Csplit or None)."""
    from vtx import ops
    c, d = case(epi, M, N, K), operands(epi, M, N, K)
    B, ntok = LAYOUT[M]
    tm = ops.tokmap(ntok)
    kw = dict(bias=d['bias'], rs=c['rs'], r_period=c['r_period'])
    if c.get('amap_tok'):
        kw['amap'] = tm
    if c['h'] is not None:
        kw.update(dgelu_in=d['h'], dgelu_kind=1)
    if c['scale'] is not None:
        kw['row_scale'] = d['scale']
    if c['R'] is not None:
        kw['R'] = d['R']
        if c['tok'] and not c['r_period']:
            kw['rmap'] = tm
        if c['rtab']:
            groups = (M - 1) // c['rtab'] + 1                                          # one spare entry behind the last group
            kw['rmap'] = ops.tabmap(c['rtab'], ops.upload_i32([TAB_STEP * g for g in range(groups + 1)], DEV), TAB_STEP)
    guards, Cs = {}, None
    if c['split_row']:
        Cs = X.sentinel_fill(torch.empty(B * T + 3, N, dtype=BF16, device=DEV))      # ldsplit = N: guard rows behind
        kw.update(split_row=c['split_row'], Csplit=Cs)
        guards['Csplit tail'] = Cs[B * T:]
    if c['tok']:
        out = X.guarded((B, 1 + ntok, N), BF16, DEV)
        kw['cmap'] = tm
        guards['cls rows'] = out[:, 0, :N]
        got = out[:, 1:, :N]
    else:
        out = X.guarded((M, N), BF16, DEV)
        got = out[:, :N]
    guards['ldc pad'] = out[..., N:]
    ops.gemm_nt(d['A'], d['W'], out, c['M'], N, K, ldc=N + 8, **kw)
    return out, got, guards, Cs


def same_bits(a, b):
    return torch.equal(a.view(torch.int16), b.view(torch.int16))


@pytest.mark.parametrize('K', [192, 256, 320])
@pytest.mark.parametrize('N', [256, 320])
@pytest.mark.parametrize('M,grid', [(600, '256'), (2360, '8'), (2360, '256')])
def test_gemm_nt_block_through_registers(M, grid, N, K, vtx_opts):
    vtx_opts('gemm_nt', 'pp256')
    vtx_opts('pp_grid', grid)
    for epi in EPILOGUES:
        c = case(epi, M, N, K)
        tag = f'block regs {epi} {M}x{N}x{K} grid={grid}'
        vtx_opts('pp_cont', '1')
        out, got, guards, Cs = launch(epi, M, N, K)
        X.check_exact(tag, got, c['expected'], guards)
        if Cs is not None:
            X.check_exact(f'{tag} Csplit', Cs[:Cs.shape[0] - 3], c['expected_split'])
        vtx_opts('pp_cont', '0')
        out2, _, _, Cs2 = launch(epi, M, N, K)
        assert same_bits(out, out2), f'{tag}: differs from the per-tile flow'
        assert Cs is None or same_bits(Cs, Cs2), f'{tag}: Csplit differs from the per-tile flow'
        print(f'{tag}: exact; identical to pp_cont=0' + (' (routed to the per-tile flow)' if epi in FALLBACK else ''))


def test_gemm_nt_block_registers_do_not_leak_between_launches(vtx_opts):
    """Five launches of the register flow on one stream, several tiles per workgroup: identical outputs."""
    vtx_opts('gemm_nt', 'pp256')
    vtx_opts('pp_grid', '8')
    vtx_opts('pp_cont', '1')
    for epi in ('residual_scale', 'mul'):
        first = launch(epi, 2360, 320, 192)[0]
        for _ in range(4):
            assert same_bits(first, launch(epi, 2360, 320, 192)[0])
