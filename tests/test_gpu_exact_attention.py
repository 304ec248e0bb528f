"""Exact-arithmetic parity of the attention and cross-attention kernels (helpers: tests/exact_attn.py, tests/exact.py).

Routed scores make softmax exact: every query has 2^k winner keys of score 0, every other key scores <= -2048, so
P in {0, 2^-k}, O = (sum of the winners' v) / 2^k and lse = k ln 2.  What each path is held to:
  MFMA kernels (bf16)      every output equals RNE(exact value): out, dq, dk, dv, the per-frame cls rows;
  VALU kernels             out equals the exact value (RNE for bf16); P stays in fp32 there and carries the lse error, so
                           dq, dk, dv lie within (8 + n) 2^-24 sum|terms| of the exact value (n = the element's non-zero
                           terms), stored: RNE of that interval for bf16 -- a single value unless it holds a bf16 rounding
                           boundary;
  lse                      exactly 0 for one winner, within 4 fp32 ulps of k ln 2 otherwise;
  probs                    zeros exact, 2^-k within 2 fp32 ulps.
Cases of kind 'graded' (forward only; tests/test_gpu_attn_graded.py) run with their own scale, c.scale, and have their own lse
standard and, on fp32 kernels, a bound on out: _check_fwd.
Outputs are written with 8 sentinel pad columns (ld_out / ld_dqkv), sentinel rows after the last sequence and a sentinel
tail on lse and probs: none of them may change.  dout carries NaN in its pad columns.  Each kernel family is forced with
the vtx_opts fixture; the comment on each test names the kernels it reaches.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import exact as X
import exact_attn as A

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
BF16, F32 = torch.bfloat16, torch.float32
PAD = 8                       # sentinel columns after every output row; sentinel rows after the last sequence


@functools.lru_cache(maxsize=None)
def contig(S, L, H, kind='exact', bwd=True, seed=0):
    return A.contig_case(S, L, H, kind, bwd, seed)


@functools.lru_cache(maxsize=None)
def space(B, T, P, H, kind='exact', bwd=True, seed=0):
    return A.space_case(B, T, P, H, kind, bwd, seed)


@functools.lru_cache(maxsize=None)
def time_cls(B, T, P, H, kind='exact', bwd=True, seed=0):
    return A.time_cls_case(B, T, P, H, kind, bwd, seed)


@functools.lru_cache(maxsize=None)
def space_nocls(B, T, P, H, kind='exact', bwd=True, seed=0):
    return A.space_nocls_case(B, T, P, H, kind, bwd, seed)


@functools.lru_cache(maxsize=None)
def cross(B, Lq, Lk, heads, hd, kind='exact', bwd=True, seed=0):
    return A.cross_case(B, Lq, Lk, heads, hd, kind, bwd, seed)


def _set(vtx_opts, opts):
    for k, v in opts.items():
        vtx_opts(k, v)


def _padded(a, dtype):
    """[rows, n] float64 -> device [rows, n + PAD] with the sentinel in the pad columns."""
    t = X.guarded(a.shape, dtype, DEV, PAD)
    t[:, :a.shape[1]] = torch.from_numpy(a).to(dtype).to(DEV)
    return t


def _lib():
    from vtx import _lib as L
    return L


def _stream():
    from vtx import ops
    return ops.stream()


def _dt(dtype):
    return _lib().VTX_F32 if dtype == F32 else _lib().VTX_BF16


def _mfma_path(c, dtype, valu):
    """Whether vtx_attn_* takes the bf16 MFMA kernels (attn.hip: attn_route, SMALL / MFMA): contig and time_cls 1..256 tokens
    (packed up to 32), space_nocls 1..256 (one tile up to 32), space 33..256."""
    if dtype != BF16 or valu:
        return False
    return c.L <= 256 and (c.layout != 'space' or c.L > 32)


def _check_bounded(name, got, c, key, dtype, guards=None):
    """VALU backward: the interval check of the module docstring."""
    exact = torch.from_numpy(getattr(c, key))
    lo, hi, b = A.value_bounds(exact, getattr(c, key + '_abs'), getattr(c, key + '_n'))
    ok = A.within(got.detach().cpu(), lo, hi, dtype)
    pinned = (X.rne_bf16(lo) == X.rne_bf16(hi)).double().mean().item() if dtype == BF16 else float((b == 0).double().mean())
    bad = ~ok
    msgs = []
    if bad.any():
        where = bad.nonzero()[:6].tolist()
        g = got.detach().cpu()
        msgs.append(f'{int(bad.sum())} of {ok.numel()} elements outside the bound; first: ' + ', '.join(
            f'{tuple(i)}: got {g[tuple(i)].item():g} exact {exact[tuple(i)].item():g} bound {b[tuple(i)].item():.3g}'
            for i in where))
    for label, region in (guards or {}).items():
        if X._sentinel_touched(region.detach()):
            msgs.append(f'guard region {label} overwritten')
    X.report(f'{"FAIL" if msgs else "ok  "} exact-bound {name}: {ok.numel()} elements, {pinned:.1%} pinned to one value'
             + (f' -- {"; ".join(msgs)}' if msgs else ''))
    assert not msgs, f'{name}: ' + '; '.join(msgs)


def _check_mask(name, ok, what):
    bad = ~ok
    X.report(f'{"FAIL" if bad.any() else "ok  "} exact {name}: {ok.numel()} elements ({what})')
    assert not bad.any(), f'{name}: {int(bad.sum())} of {ok.numel()} outside ({what}); first {bad.nonzero()[:6].tolist()}'


def _check_fwd(name, c, dtype, out, out_guards, lse, lse_name=None):
    """out and lse (device views of the compared elements) against the case.  Graded cases (exact_attn.py: 'graded'): the lse
    standard is lse_graded_ok, and fp32 kernels, whose P stays fp32, are held to value_bounds on out (how many elements equal
    the exact value is reported, not asserted)."""
    if c.kind == 'graded' and dtype == F32:
        _check_bounded(name, out, c, 'out', dtype, out_guards)
        want = torch.from_numpy(c.out).float()
        X.report(f'ok   graded fp32 {name}: {int(X.mismatch(out.detach().cpu(), want).sum())} of {want.numel()} elements differ from '
                 f'the exact value')
    else:
        X.check_exact(name, out, A.expect(name, c.out, dtype, c.kind), out_guards)
    name = lse_name or name
    if c.kind == 'graded':
        _check_mask(f'{name} lse', A.lse_graded_ok(lse.cpu(), c.log2l.reshape(-1), c.top.reshape(-1)),
                    '4 ulps at k ln2 + 2 ulps at top ln2 of (k - top) ln2')
    else:
        _check_mask(f'{name} lse', A.lse_ok(lse.cpu(), c.nwin.reshape(-1)), '0 for one winner, 4 ulps of k ln2')


# ------------------------------------------------------------------------------------------------ self-attention
QKV_PAD = {'contig': 0, 'space': 0, 'time_cls': PAD, 'space_nocls': PAD}      # NaN columns after every row of qkv


def attn_desc(c, dtype, qkv, out, lse, probs=None):
    L = _lib()
    d = L.AttnDesc()
    d.dtype = _dt(dtype)
    d.mode = {'contig': L.ATTN_CONTIG, 'space': L.ATTN_SPACE, 'time_cls': L.ATTN_TIME_CLS,
              'space_nocls': L.ATTN_SPACE_NOCLS}[c.layout]
    d.S, d.L, d.H, d.hd = c.S, c.L, c.H, c.hd
    d.B, d.T, d.P = c.B, c.T, c.P
    d.qkv, d.ld_qkv = qkv.data_ptr(), qkv.stride(0)
    D = c.H * c.hd
    d.out, d.ld_out = out.data_ptr(), D + PAD
    d.lse = lse.data_ptr()
    d.probs = None if probs is None else probs.data_ptr()
    d.scale = c.scale
    return d


def _shape(c):
    btp = '' if c.layout == 'contig' else f' B={c.B} T={c.T} P={c.P}'
    return f'{c.layout}{btp} S={c.S} L={c.L} H={c.H}' + ('' if c.hd == 64 else f' hd={c.hd}')


def run_fwd(c, dtype, probs=False):
    """Forward with guarded outputs; checks out, lse (and probs).  Returns (qkv, out, lse) device tensors.  In the
    time_cls and space_nocls layouts qkv has PAD columns of NaN after every row (ld_qkv = 3D + PAD): a kernel that takes
    ld_qkv for 3D reads them."""
    D, n = c.H * c.hd, c.S * c.H * c.L
    qkv = torch.full((c.qkv.shape[0], 3 * D + QKV_PAD[c.layout]), float('nan'), dtype=dtype, device=DEV)
    qkv[:, :3 * D] = torch.from_numpy(c.qkv).to(dtype).to(DEV)
    rows = c.out.shape[0]
    out = X.guarded((rows + 2, D), dtype, DEV, PAD)
    lse = X.sentinel_fill(torch.empty(n + PAD, device=DEV))
    pr = X.sentinel_fill(torch.empty(n * c.L + PAD, device=DEV)) if probs else None
    d = attn_desc(c, dtype, qkv, out, lse, pr)
    _lib().call('vtx_attn_fwd', C.byref(d), _stream())
    torch.cuda.synchronize()
    name = f'attn fwd {_shape(c)} {c.kind} {dtype}'
    _check_fwd(name, c, dtype, out[:rows, :D], {'ld_out pad': out[:, D:], 'rows after the last sequence': out[rows:, :D]}, lse[:n])
    X.check_exact(f'{name} lse tail', lse[n:], lse[n:].cpu(), {'lse tail': lse[n:]})
    if probs:
        assert c.kind != 'graded'
        # probs is [S, H, L, L] whatever the layout: the block of item n = s H + h is indexed by the positions i, j in
        # the sequence, not by the rows they sit on
        want = np.zeros((c.S * c.H, c.L, c.L))
        it = c.items
        i_idx = np.arange(c.L)[None, :, None].repeat(it.I, 0).repeat(4, 2)
        s_idx = np.arange(it.I)[:, None, None].repeat(c.L, 1).repeat(4, 2)
        v = it.win >= 0
        want[s_idx[v], i_idx[v], it.win[v]] = 1.0 / it.nwin[..., None].repeat(4, 2)[v]
        _check_mask(f'{name} probs', A.probs_ok(pr[:n * c.L].cpu(), torch.from_numpy(want.reshape(-1))),
                    'zeros exact, 2^-k within 2 ulps')
        X.check_exact(f'{name} probs tail', pr[n * c.L:], pr[n * c.L:].cpu(), {'probs tail': pr[n * c.L:]})
    return qkv, out, lse


def run_bwd(c, dtype, qkv, out, lse, exact):
    """Backward from the forward's own out / lse; checks dqkv and, where c.cls_group sequences share a cls row (space,
    time_cls), dqkv_cls (one row per sequence), the untouched cls rows and cls_qkv_reduce over c.cls_group rows.  space_nocls
    passes no dqkv_cls, and the cls rows of dqkv must hold +0 over exactly 3D columns.  exact: RNE equality (MFMA) or the
    interval check (VALU).  Returns the device outputs."""
    L_ = _lib()
    D = c.H * c.hd
    W = 3 * D
    rows = c.qkv.shape[0]
    dout = _padded(c.dout, dtype)
    dqkv = X.guarded((rows + 2, W), dtype, DEV, PAD)
    b = L_.AttnBwdDesc()
    b.f = attn_desc(c, dtype, qkv, out, lse)
    b.dout, b.ld_dout = dout.data_ptr(), D + PAD
    b.dqkv, b.ld_dqkv = dqkv.data_ptr(), W + PAD
    delta = torch.empty(c.S * c.H * c.L, device=DEV)
    b.delta = delta.data_ptr()
    dcls = None
    if c.cls_group:
        dcls = X.guarded((c.S + 2, W), dtype, DEV, PAD)
        b.dqkv_cls = dcls.data_ptr()
    else:
        b.dqkv_cls = None
    L_.call('vtx_attn_bwd', C.byref(b), _stream())
    torch.cuda.synchronize()
    name = f'attn bwd {_shape(c)} {dtype}'
    guards = {'ld_dqkv pad': dqkv[:, W:], 'rows after the last sequence': dqkv[rows:, :W]}
    if c.cls_group:
        tok = torch.from_numpy(~np.isnan(c.dqkv[:, 0]))
        cls_rows = torch.nonzero(~tok).reshape(-1)
        assert cls_rows.tolist() == c.cls_rows.tolist()
        guards['clip cls rows'] = dqkv[cls_rows.to(DEV), :W]
        got_tok = dqkv[:rows, :W][tok.to(DEV)]
        sub = {k: getattr(c, 'dqkv' + k)[tok.numpy()] for k in ('', '_abs', '_n')}
    else:
        got_tok, sub = dqkv[:rows, :W], {k: getattr(c, 'dqkv' + k) for k in ('', '_abs', '_n')}
    if c.layout == 'space_nocls':
        # the cls rows of dqkv: +0 bit for bit over exactly 3D columns (check_exact lets -0 pass for 0), their pad columns
        # still the sentinel
        cls_rows = torch.from_numpy(c.cls_rows).to(DEV)
        zrows = dqkv[cls_rows]
        nz = int((zrows[:, :W].contiguous().view(torch.int16 if dtype == BF16 else torch.int32) != 0).sum())
        touched = X.sentinel_touched(zrows[:, W:])
        ok = nz == 0 and touched == 0
        X.report(f'{"ok  " if ok else "FAIL"} exact {name} cls rows of dqkv: {zrows[:, :W].numel()} elements (+0), '
                 f'{nz} not +0, {touched} pad elements overwritten')
        assert ok, f'{name}: cls rows of dqkv: {nz} elements are not +0, {touched} pad elements overwritten'
    _check_self_grad(name, got_tok, sub, dtype, exact, guards)
    if c.cls_group:
        csub = {k: getattr(c, 'dqkv_cls' + k) for k in ('', '_abs', '_n')}
        _check_self_grad(f'{name} per-frame cls rows', dcls[:c.S, :W], csub, dtype, exact,
                         {'ld_dqkv pad': dcls[:, W:], 'rows after the last frame': dcls[c.S:, :W]})
        # cls_qkv_reduce: fp32 sum of the stored rows of the cls_group sequences that share the cls row, in sequence order,
        # stored once (vtx.h)
        rpc = 1 + c.P * c.T
        L_.call('vtx_cls_qkv_reduce', _dt(dtype), c.B, c.cls_group, W, dcls.data_ptr(), W + PAD, dqkv.data_ptr(), W + PAD, rpc,
                _stream())
        torch.cuda.synchronize()
        frames = dcls[:c.S, :W].cpu().float().reshape(c.B, c.cls_group, W)
        acc = torch.zeros(c.B, W)
        for t in range(c.cls_group):
            acc = acc + frames[:, t]
        X.check_exact(f'{name} cls_qkv_reduce', dqkv[cls_rows.to(DEV), :W], acc.to(dtype),
                      {'ld_dqkv pad': dqkv[:, W:]})
    return dqkv, dcls


def _check_self_grad(name, got, sub, dtype, exact, guards):
    if exact:
        X.check_exact(name, got, A.expect(name, sub[''], dtype, None), guards)
        return
    holder = type('H', (), {})()
    holder.g, holder.g_abs, holder.g_n = sub[''], sub['_abs'], sub['_n']
    _check_bounded(name, got, holder, 'g', dtype, guards)


def run_self(c, dtype, valu=False, probs=False):
    qkv, out, lse = run_fwd(c, dtype, probs)
    res = (out, lse)
    if c.bwd:
        res += run_bwd(c, dtype, qkv, out, lse, _mfma_path(c, dtype, valu))
    return res


# attn_fwd_small_kernel<HW>, attn_bwd_small_kernel<HW>: bf16, contig, L <= 32.  attn_hw_* = 0: one head, four row tiles per
# workgroup (<false>); n > 0: n heads of one tile (<true>).  S = 37 is not a multiple of 32 / L for any L here; H = 5 does not
# divide into groups of 3 or 16.
@pytest.mark.parametrize('hw', ['0', '3', '16'])
@pytest.mark.parametrize('L', [1, 5, 8, 9, 17, 32])
def test_attn_small_kernels_exact(L, hw, vtx_opts):
    vtx_opts('attn_hw_fwd', hw)
    vtx_opts('attn_hw_bwd', hw)
    run_self(contig(37, L, 5), BF16)


# attn_fwd_mfma_kernel<0> (L 33..192, 225..256) and <7> with attn_fwd_stream=0 (L 193..224); the default backward of each L:
# attn_bwd_fused_mfma_kernel<0> (33..192), attn_bwd_stream_mfma_kernel<7> (193..224), the dq + dkv pair <0> (225..256).
@pytest.mark.parametrize('L', [33, 65, 130, 193, 197, 224, 256])
def test_attn_mfma_forward_exact(L, vtx_opts):
    vtx_opts('attn_fwd_stream', '0')
    run_self(contig(3, L, 3), BF16)


# attn_fwd_stream_mfma_kernel<7> + attn_bwd_stream_mfma_kernel<7> (the defaults for 193..224 tokens) with S*H > 256 items, so
# every persistent workgroup handles several: contig 70 x 12 and space B=6 T=8 P=196.  Consecutive items draw their group
# codes independently: a stale K / V row of the previous item scores 0 with some query.  A second run is bit-identical.
@pytest.mark.parametrize('layout', ['contig', 'space'])
def test_attn_streamed_bench_scale_exact(layout):
    c = contig(70, 197, 12) if layout == 'contig' else space(6, 8, 196, 12)
    first = run_self(c, BF16)
    again = run_self(c, BF16)
    for a, b in zip(first, again):
        if a is not None:
            assert torch.equal(a.view(torch.int16) if a.dtype == BF16 else a.view(torch.int32),
                               b.view(torch.int16) if b.dtype == BF16 else b.view(torch.int32)), 'second run differs'


# attn_bwd_fused_mfma_kernel<0> / <7>: attn_fused=1 (one persistent pass, two phases).  A second run is bit-identical.
@pytest.mark.parametrize('L', [33, 130, 197])
def test_attn_bwd_fused_exact(L, vtx_opts):
    vtx_opts('attn_fused', '1')
    c = contig(5, L, 3)
    first = run_self(c, BF16)
    again = run_self(c, BF16)
    assert torch.equal(first[2].view(torch.int16), again[2].view(torch.int16)), 'second run differs'


# attn_bwd_dq_mfma_kernel + attn_bwd_dkv_mfma_kernel: attn_fused=0, all five attn_dkv variants at L = 197 (<7, 0, 0>,
# <7, 7, 1>, <7, 7, 0>, <7, 7, 2>, <7, 7, 3>), and the run-time tile loop <0, 0, 0> at L = 37 and 256.
@pytest.mark.parametrize('L,dkv', [(197, '0'), (197, '1'), (197, '2'), (197, '3'), (197, '4'), (37, '3'), (256, '3')])
def test_attn_bwd_pair_exact(L, dkv, vtx_opts):
    vtx_opts('attn_fused', '0')
    vtx_opts('attn_dkv', dkv)
    run_self(contig(4, L, 3), BF16)


# VALU attn_fwd_kernel / attn_bwd_dq_kernel / attn_bwd_dkv_kernel: fp32; bf16 with attn_valu=1; bf16 above 256 tokens.
# L <= 64 packs G = 128 / L sequences per workgroup (S = 37: not a multiple of G); 65..256 has a ragged 64-key tile.
@pytest.mark.parametrize('L', [8, 37, 130, 300])
@pytest.mark.parametrize('mode', ['f32', 'bf16_valu'])
def test_attn_valu_exact(mode, L, vtx_opts):
    dtype = F32 if mode == 'f32' else BF16
    if mode == 'bf16_valu':
        vtx_opts('attn_valu', '1')
    run_self(contig(37 if L <= 64 else 3, L, 2), dtype, valu=True)


def test_attn_valu_bf16_long_exact():
    """bf16 above 256 tokens runs the VALU kernels whatever the options."""
    run_self(contig(2, 300, 2, seed=3), BF16, valu=True)


# probs= (attn_fwd_kernel<T, 64, 1> after the forward): contig L = 197 and 9, both dtypes.
@pytest.mark.parametrize('dtype', [F32, BF16])
@pytest.mark.parametrize('L', [9, 197])
def test_attn_probs_exact(L, dtype):
    run_self(contig(3, L, 2, seed=5), dtype, valu=dtype == F32, probs=True)


# VTX_ATTN_SPACE: P + 1 <= 32 runs the VALU kernels, 33..256 the MFMA kernels (bf16; <0> for 37, the streamed <7> for 197).
@pytest.mark.parametrize('dtype', [F32, BF16])
@pytest.mark.parametrize('B,T,P', [(2, 3, 8), (2, 3, 36), (2, 3, 196)])
def test_attn_space_exact(B, T, P, dtype):
    c = space(B, T, P, 2)
    run_self(c, dtype, valu=dtype == F32)


# Forward "round" cases: V in 128..255, so a share of the outputs are exact ties and most are inexact: RNE at the O store of
# every family.
ROUND = {
    'small<true>': (lambda: contig(37, 8, 5, 'round', False), BF16, {}),
    'small<false>': (lambda: contig(37, 8, 5, 'round', False), BF16, {'attn_hw_fwd': '0'}),
    'mfma<0>': (lambda: contig(3, 130, 3, 'round', False), BF16, {}),
    'mfma<7>': (lambda: contig(3, 197, 3, 'round', False), BF16, {'attn_fwd_stream': '0'}),
    'stream<7>': (lambda: contig(3, 197, 3, 'round', False), BF16, {}),
    'valu bf16': (lambda: contig(3, 130, 3, 'round', False), BF16, {'attn_valu': '1'}),
    'valu bf16 packed': (lambda: contig(37, 8, 5, 'round', False), BF16, {'attn_valu': '1'}),
    'space mfma': (lambda: space(2, 3, 36, 2, 'round', False), BF16, {}),
    'space valu': (lambda: space(2, 3, 8, 2, 'round', False), BF16, {}),
}


@pytest.mark.parametrize('family', list(ROUND))
def test_attn_forward_round_exact(family, vtx_opts):
    make, dtype, opts = ROUND[family]
    _set(vtx_opts, opts)
    run_self(make(), dtype)


# ------------------------------------------------------------------------------------------------ cross attention
def xattn_desc(c, dtype, q, k, v, out, lse):
    L = _lib()
    d = L.XAttnDesc()
    d.dtype = _dt(dtype)
    d.B, d.Lq, d.Lk, d.heads, d.hd = c.B, c.Lq, c.Lk, c.H, c.hd
    d.scale = c.scale                               # SCALE: a power of two also for head_dim 96 (XAttnFn uses hd^-0.5)
    d.q, d.k, d.v, d.out, d.lse = q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), lse.data_ptr()
    return d


def _tailed(shape, dtype):
    """Sentinel-filled flat buffer of prod(shape) + PAD * 8 elements: (view of shape, tail)."""
    n = int(np.prod(shape))
    buf = X.sentinel_fill(torch.empty(n + PAD * 8, dtype=dtype, device=DEV))
    return buf[:n].view(*shape), buf[n:]


def run_cross(c, dtype, exact_bwd):
    L = _lib()
    C_ = c.H * c.hd
    q, k, v = (torch.from_numpy(a).to(dtype).to(DEV).contiguous() for a in (c.q, c.k, c.v))
    out, out_t = _tailed((c.B, c.Lq, C_), dtype)
    lse, lse_t = _tailed((c.B * c.H * c.Lq,), F32)
    d = xattn_desc(c, dtype, q, k, v, out, lse)
    L.call('vtx_xattn_fwd', C.byref(d), _stream())
    torch.cuda.synchronize()
    name = f'xattn B={c.B} Lq={c.Lq} Lk={c.Lk} heads={c.H} hd={c.hd} {c.kind} {dtype}'
    _check_fwd(f'{name} out', c, dtype, out, {'tail': out_t}, lse, name)
    X.check_exact(f'{name} lse tail', lse_t, lse_t.cpu(), {'tail': lse_t})
    if not c.bwd:
        return out, lse
    dout = torch.from_numpy(c.dout).to(dtype).to(DEV).contiguous()
    dq, dq_t = _tailed((c.B, c.Lq, C_), dtype)
    dk, dk_t = _tailed((c.B, c.Lk, C_), dtype)
    dv, dv_t = _tailed((c.B, c.Lk, C_), dtype)
    delta = torch.empty(c.B * c.H * c.Lq, device=DEV)
    ws_bytes = L.load().vtx_xattn_bwd_workspace(C.byref(d))
    ws = torch.empty(max(ws_bytes // 4, 4), device=DEV)
    L.call('vtx_xattn_bwd', C.byref(d), dout.data_ptr(), delta.data_ptr(), dq.data_ptr(), dk.data_ptr(), dv.data_ptr(),
           ws.data_ptr(), ws_bytes, _stream())
    torch.cuda.synchronize()
    for key, got, tail in (('dq', dq, dq_t), ('dk', dk, dk_t), ('dv', dv, dv_t)):
        if exact_bwd:
            X.check_exact(f'{name} {key}', got, A.expect(name, getattr(c, key), dtype, None), {'tail': tail})
        else:
            _check_bounded(f'{name} {key}', got, c, key, dtype, {'tail': tail})


# xattn_mfma.hip fwd_kernel / bwd_dq_kernel / bwd_dkv_kernel + the split reduction: bf16, head_dim 64 and 96, ragged Lk
# (37, 393), Lq >> Lk so the dk / dv kernel runs several query splits (2500 x 393).
@pytest.mark.parametrize('hd', [64, 96])
@pytest.mark.parametrize('B,Lq,Lk', [(2, 300, 37), (1, 2500, 393)])
def test_xattn_mfma_exact(B, Lq, Lk, hd):
    run_cross(cross(B, Lq, Lk, 2, hd), BF16, True)


# The VALU cross attention of mvit.hip: fp32, and bf16 with attn_valu=1.
@pytest.mark.parametrize('hd', [64, 96])
@pytest.mark.parametrize('mode', ['f32', 'bf16_valu'])
@pytest.mark.parametrize('B,Lq,Lk', [(2, 300, 37), (1, 2500, 393)])
def test_xattn_valu_exact(B, Lq, Lk, mode, hd, vtx_opts):
    if mode == 'bf16_valu':
        vtx_opts('attn_valu', '1')
    run_cross(cross(B, Lq, Lk, 2, hd), F32 if mode == 'f32' else BF16, False)


@pytest.mark.parametrize('hd', [64, 96])
def test_xattn_forward_round_exact(hd, vtx_opts):
    c = cross(2, 300, 37, 2, hd, 'round', False)
    run_cross(c, BF16, True)
    vtx_opts('attn_valu', '1')
    run_cross(c, BF16, False)
