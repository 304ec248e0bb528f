"""Divided attention in space-then-time order: operator_order = ['space_attn', 'time_attn', 'ffn'], where the spatial block
runs without the cls token (VTX_ATTN_SPACE_NOCLS, vtx.functions.AttnFn kind 'space_nocls') and the temporal block over it
(VTX_ATTN_TIME_CLS, kind 'time_cls').  Reference transformer.py:238-282, :340-382, :602,611.

  1. model-level parity against the goldens of the running reference (tests/golden/make_golden_cls_order.py): fp32 within
     TOL_F32; bf16 within TOL_BF16 / TOL_BF16_GRAD, widened per tensor to AUTOCAST_FACTOR x the reference's own autocast
     deviation (tests/golden/cls_order_cal.json) and capped at WIDEN_CAP -- helpers.check / helpers.compare_grads.  The DropPath
     case keeps the FIXED bars: the reference's autocast run draws its DropPath masks in bfloat16, so it drops other sequences
     than its fp32 run and its deviation (1.8e-1 on the outputs) calibrates nothing;
  2. both layouts of vtx_attn_fwd / vtx_attn_bwd against a float64 evaluation of the same regrouping, at the lengths that
     select each kernel family, bf16 and fp32: TOL[dtype] on out, 1e-4 on lse, 2 TOL[dtype] on dqkv and the per-sequence cls
     rows (the bars of tests/test_gpu_long_attention.py and tests/test_gpu_f32_attention.py);
  3. attn_f32=valu against mfma and attn_long=0 against 1 on the new layouts (the bars of those files' option tests);
  4. recompute against stored activations, bit for bit, and the direct-gradient path against autograd's accumulation;
  5. exact arithmetic (tests/exact_attn.py: routed inputs whose results have one correct bf16 value each) for the packed
     TIME_CLS kernels at L = 9 and 17, with one head and with several heads per workgroup: out, lse, dqkv and dqkv_cls are
     compared for equality, so a cls row gathered from or scattered to the wrong row shows as such, not as rounding.  The
     other kernel families of the two layouts are held to the same standard in tests/test_gpu_exact_attn_layouts.py.
"""
import json
import os

import numpy as np
import pytest
import torch

import helpers
from helpers import GOLD, TOL_BF16, TOL_BF16_GRAD, TOL_F32, check, compare_grads, gold
from oracle import synth
from oracle.synth import synth_tensor
from test_gpu_kernels import TOL, dev, rnd

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
BF16, F32 = torch.bfloat16, torch.float32
LSE_BAR = 1e-4
ORDER = ['space_attn', 'time_attn', 'ffn']
D, HEADS, HIDDEN = 128, 2, 256
# the cases of tests/golden/make_golden_cls_order.py: (clips, T, P, layers, drop_path_rate, mode), seeds in the same order
CASES = {
    't8_p16': (2, 8, 16, 1, 0.0, 'train'),
    't8_p196': (1, 8, 196, 1, 0.0, 'train'),
    't32_p16': (2, 32, 16, 1, 0.0, 'train'),
    't8_p16_eval_attn': (2, 8, 16, 2, 0.0, 'eval'),
    't8_p16_droppath': (4, 8, 16, 2, 0.3, 'train'),
}
SEED = {name: 11 + i for i, name in enumerate(CASES)}


@pytest.fixture(autouse=True)
def _defaults():
    import vtx
    # the calibration of these cases lives in its own file; helpers.cal_entry reads one table
    helpers._CAL = dict(json.load(open(os.path.join(GOLD, 'autocast_cal.json'))), **json.load(open(os.path.join(GOLD, 'cls_order_cal.json'))))
    yield
    helpers._CAL = None
    vtx.set_precision('auto')
    vtx.set_stream('bf16')
    vtx.set_recompute(False)


def _container(name):
    import transformer as T_
    B, T, P, layers, dpr, mode = CASES[name]
    m = T_.TransformerContainer(num_transformer_layers=layers, embed_dims=D, num_heads=HEADS, num_frames=T,
                                hidden_channels=HIDDEN, operator_order=list(ORDER), drop_path_rate=dpr)
    m.load_state_dict(synth.synth_state_dict(synth.shapes_of(m), SEED[name]), strict=True)
    x = torch.from_numpy(np.random.RandomState(SEED[name]).standard_normal((B, 1 + P * T, D)).astype(np.float32))
    return m.to(DEV), x.to(DEV)


def _step(m, x, seed):
    import transformer as T_
    m.train()
    m.zero_grad()
    torch.manual_seed(seed)
    y = T_.stream_value(m(x)).float()                # (the exact stream hands on contributions: the stream itself)
    w = (synth_tensor('loss_w', (D,), 0) * 10.0).to(DEV)
    (y * w).sum().backward()
    torch.cuda.synchronize()
    return y.detach(), {k: p.grad for k, p in m.named_parameters() if p.grad is not None}


def _check_out(tag, y, g, tol, cal):
    if 'out' in g.files:
        check(tag + ' out', y.cpu(), g['out'], tol, cal=cal)
    else:
        flat = y.cpu().flatten()
        check(tag + ' out (samples)', flat[helpers.sample_idx(flat.numel())], g['outs'], tol, cal=cal)


PRECS = [('fp32', TOL_F32, TOL_F32, 'bf16'), ('bf16', TOL_BF16, TOL_BF16_GRAD, 'bf16'), ('bf16', TOL_BF16, TOL_BF16_GRAD, 'fp32')]


@pytest.mark.parametrize('prec,tol,gtol,stream', PRECS, ids=['fp32', 'bf16', 'bf16-exact-stream'])
@pytest.mark.parametrize('name', ['t8_p16', 't8_p196', 't32_p16', 't8_p16_droppath'])
def test_train_step_against_the_reference(name, prec, tol, gtol, stream):
    import vtx
    vtx.set_precision(prec)
    vtx.set_stream(stream)
    m, x = _container(name)
    y, grads = _step(m, x, SEED[name])
    g = gold(f'cls_order_{name}.npz')
    cal = 'cls_order ' + name if (prec == 'bf16' and name != 't8_p16_droppath') else None
    tag = f'cls order {name} {prec} stream={stream}'
    _check_out(tag, y, g, tol, cal)
    assert len(grads) == len(list(m.parameters()))
    compare_grads(tag, grads, g, gtol, exact_elements=(prec == 'fp32'), cal=cal)


@pytest.mark.parametrize('prec,tol,stream', [('fp32', TOL_F32, 'bf16'), ('bf16', TOL_BF16, 'bf16'), ('bf16', TOL_BF16, 'fp32')],
                         ids=['fp32', 'bf16', 'bf16-exact-stream'])
def test_eval_and_return_attention_against_the_reference(prec, tol, stream):
    """Eval forward of two layers, and the weights of the block's last attention: the temporal one, [(b p), H, T+1, T+1]."""
    import vtx
    import transformer as T_
    name = 't8_p16_eval_attn'
    vtx.set_precision(prec)
    vtx.set_stream(stream)
    m, x = _container(name)
    m.eval()
    g = gold(f'cls_order_{name}.npz')
    with torch.no_grad():
        y = T_.stream_value(m(x)).float()
        a = m(x, return_attention=True).float()
    B, T, P = CASES[name][:3]
    assert tuple(a.shape) == (B * P, HEADS, T + 1, T + 1)
    cal = 'cls_order ' + name if prec == 'bf16' else None
    _check_out(f'cls order {name} {prec} stream={stream}', y, g, tol, cal)
    e = helpers.relerr(a.cpu(), g['attn'])
    bar = tol if cal is None else max(tol, min(helpers.AUTOCAST_FACTOR * helpers.cal_entry(cal)['attn'], helpers.WIDEN_CAP * tol))
    helpers.report(f'{"ok  " if e <= bar else "FAIL"} cls order {name} {prec} stream={stream} attention: rel={e:.3e} (tol {bar:g})')
    assert e <= bar, f'attention weights: {e:.3e} > {bar:g}'


# ------------------------------------------------------------------------------------------------ 2. kernels vs float64
def _ref(seqs, H):
    """[S, L, 3D] float64 -> out [S, L, D], lse [S, H, L]"""
    S, L, D3 = seqs.shape
    hd = D3 // 3 // H
    t = seqs.reshape(S, L, 3, H, hd)
    qq, kk, vv = (t[:, :, i].permute(0, 2, 1, 3) for i in range(3))
    sc = qq @ kk.transpose(-1, -2) * hd ** -0.5
    o = (torch.softmax(sc, -1) @ vv).permute(0, 2, 1, 3).reshape(S, L, D3 // 3)
    return o, torch.logsumexp(sc, -1)


def _run(mode, qkv, do, B, T, P, H, dtype):
    """(out, lse, dqkv, dqkv_cls or None); every buffer starts as NaN: a row the kernels skip shows"""
    from vtx import ops
    from vtx import _lib
    hd, Dm, N = 64, H * 64, P * T
    if mode == 'time_cls':
        code, S, L, extra = _lib.ATTN_TIME_CLS, B * P, T + 1, B * P
    else:
        code, S, L, extra = _lib.ATTN_SPACE_NOCLS, B * T, P, 0
    o = torch.full((B * N + extra, Dm), float('nan'), dtype=dtype, device=DEV)
    lse = torch.full((S * H * L,), float('nan'), device=DEV)
    ops.attn_fwd(qkv, o, lse, code, S, L, H, hd, hd ** -0.5, B, T, P)
    dqkv = torch.full((B, 1 + N, 3 * Dm), float('nan'), dtype=dtype, device=DEV)
    dcls = torch.full((B * P, 3 * Dm), float('nan'), dtype=dtype, device=DEV) if extra else None
    ops.attn_bwd(qkv, o, lse, do, dqkv, code, S, L, H, hd, hd ** -0.5, B, T, P, dqkv_cls=dcls)
    torch.cuda.synchronize()
    return o, lse.reshape(S, H, L), dqkv, dcls


def _inputs(mode, B, T, P, H, dtype):
    Dm, N = H * 64, P * T
    qkv = rnd(B, 1 + N, 3 * Dm, seed=5) * 1.5
    do = rnd(B * N + (B * P if mode == 'time_cls' else 0), Dm, seed=6)
    return qkv, do


def _against_f64(mode, B, T, P, H, dtype, tag):
    Dm, N = H * 64, P * T
    qkv, do = _inputs(mode, B, T, P, H, dtype)
    qd = dev(qkv, dtype)
    if mode == 'space_nocls':
        qd[:, 0] = float('nan')                                  # the cls rows of qkv are not read
    o, lse, dqkv, dcls = _run(mode, qd, dev(do, dtype), B, T, P, H, dtype)
    q64, do64 = qkv.to(dtype).double(), do.to(dtype).double()
    tok = q64[:, 1:].reshape(B, P, T, 3 * Dm)
    if mode == 'time_cls':
        seqs = torch.cat((q64[:, :1].unsqueeze(1).expand(B, P, 1, 3 * Dm), tok), 2).reshape(B * P, T + 1, 3 * Dm)
    else:
        seqs = tok.permute(0, 2, 1, 3).reshape(B * T, P, 3 * Dm)
    seqs = seqs.clone().requires_grad_(True)
    ro, rlse = _ref(seqs, H)
    if mode == 'time_cls':
        r_tok, r_cls = ro[:, 1:].reshape(B * N, Dm), ro[:, 0]
        ((r_tok * do64[:B * N]).sum() + (r_cls * do64[B * N:]).sum()).backward()
        g_tok, g_cls = seqs.grad[:, 1:].reshape(B, N, 3 * Dm), seqs.grad[:, 0]
        check(f'{tag} fwd cls rows', o[B * N:].float().cpu(), r_cls.detach(), TOL[dtype])
        check(f'{tag} bwd cls rows', dcls.float().cpu(), g_cls, 2 * TOL[dtype])
    else:
        r_tok = ro.reshape(B, T, P, Dm).permute(0, 2, 1, 3).reshape(B * N, Dm)
        (r_tok * do64).sum().backward()
        g_tok = seqs.grad.reshape(B, T, P, 3 * Dm).permute(0, 2, 1, 3).reshape(B, N, 3 * Dm)
        assert torch.equal(dqkv[:, 0].float().cpu(), torch.zeros(B, 3 * Dm)), 'the cls rows of dqkv are zeros'
    check(f'{tag} fwd tokens', o[:B * N].float().cpu(), r_tok.detach(), TOL[dtype])
    check(f'{tag} lse', lse.cpu(), rlse.detach(), LSE_BAR)
    check(f'{tag} bwd tokens', dqkv[:, 1:].float().cpu(), g_tok, 2 * TOL[dtype])


@pytest.mark.parametrize('dtype', [BF16, F32], ids=['bf16', 'fp32'])
@pytest.mark.parametrize('B,T,P', [(3, 8, 7), (2, 16, 5), (2, 32, 3), (2, 96, 2), (1, 8, 196)],
                         ids=['L9', 'L17', 'L33', 'L97', 'L9-p196'])
def test_time_cls_against_float64(B, T, P, dtype):
    """L = T + 1 = 9, 17: the packed kernels (bf16; 3 and 1 sequences per 32-row tile, the last tile ragged) / VALU (fp32);
    33, 97: one workgroup per (sequence, head) (bf16) / the exact-fp32 MFMA kernels."""
    _against_f64('time_cls', B, T, P, 3, dtype, f'attn time_cls B{B} T{T} P{P} {str(dtype)[6:]}')


@pytest.mark.parametrize('dtype', [BF16, F32], ids=['bf16', 'fp32'])
@pytest.mark.parametrize('B,T,P', [(3, 4, 16), (2, 3, 196), (1, 2, 784)], ids=['L16', 'L196', 'L784'])
def test_space_nocls_against_float64(B, T, P, dtype):
    """L = P = 16: one workgroup per (sequence, head) at a single tile (bf16) / VALU (fp32); 196: the same family with seven
    tiles and a row stride; 784: the chunk-streaming kernels."""
    _against_f64('space_nocls', B, T, P, 3, dtype, f'attn space_nocls B{B} T{T} P{P} {str(dtype)[6:]}')


# ------------------------------------------------------------------------------------------------ 3. options
SHAPES = [('time_cls', 2, 32, 3), ('time_cls', 2, 8, 5), ('space_nocls', 2, 3, 196), ('space_nocls', 1, 2, 784)]


def _pair(mode, B, T, P, dtype, flip):
    qkv, do = _inputs(mode, B, T, P, 3, dtype)
    qd, dd = dev(qkv, dtype), dev(do, dtype)
    new = _run(mode, qd, dd, B, T, P, 3, dtype)
    flip()
    old = _run(mode, qd, dd, B, T, P, 3, dtype)
    return [(a.float().cpu(), b.float().cpu()) for a, b in zip(new, old) if a is not None]


@pytest.mark.parametrize('mode,B,T,P', SHAPES)
def test_attn_f32_valu_agrees_with_mfma(mode, B, T, P):
    import vtx
    try:
        pairs = _pair(mode, B, T, P, F32, lambda: vtx.set_option('attn_f32', 'valu'))
    finally:
        vtx.set_option('attn_f32', 'mfma')
    for what, (a, b), bar in zip(('out', 'lse', 'dqkv', 'dqkv_cls'), pairs, (TOL[F32], LSE_BAR, 2 * TOL[F32], 2 * TOL[F32])):
        check(f'attn f32 mfma vs valu {what} {mode} B{B} T{T} P{P}', torch.nan_to_num(a), torch.nan_to_num(b), bar)


@pytest.mark.parametrize('mode,B,T,P', SHAPES)
def test_attn_long_0_agrees_with_1(mode, B, T, P):
    import vtx
    try:
        pairs = _pair(mode, B, T, P, BF16, lambda: vtx.set_option('attn_long', '0'))
    finally:
        vtx.set_option('attn_long', '1')
    for what, (a, b), bar in zip(('out', 'lse', 'dqkv', 'dqkv_cls'), pairs, (1e-2, 1e-4, 2e-2, 2e-2)):
        check(f'attn long vs valu {what} {mode} B{B} T{T} P{P}', torch.nan_to_num(a), torch.nan_to_num(b), bar)


# ------------------------------------------------------------------------------------------------ 4. recompute, direct gradients
def test_recompute_equals_stored_activations():
    """Two layers with DropPath: the re-run draws the same masks; outputs and gradients bit for bit."""
    import vtx
    vtx.set_precision('bf16')
    res = []
    for rc in (False, True):
        vtx.set_recompute(rc)
        m, x = _container('t8_p16_droppath')
        y, grads = _step(m, x, 21)
        res.append((y.clone(), {k: v.clone() for k, v in grads.items()}))
    assert torch.equal(res[0][0], res[1][0])
    assert set(res[0][1]) == set(res[1][1])
    for k in res[0][1]:
        assert torch.equal(res[0][1][k], res[1][1][k]), k


@pytest.mark.parametrize('prec', ['bf16', 'fp32'])
def test_direct_gradients_equal_autograd(prec):
    import vtx
    from vtx import dp, functions
    vtx.set_precision(prec)
    m, x = _container('t8_p16_droppath')
    _, ref = _step(m, x, 21)
    ref = {k: v.clone() for k, v in ref.items()}
    for recompute in (False, True):
        vtx.set_recompute(recompute)
        buckets = dp.GradBuckets(list(m.parameters()), bucket_bytes=64 << 10, direct=True)
        try:
            assert functions.direct_grads_enabled()
            buckets.zero()
            m.train()
            torch.manual_seed(21)
            w = (synth_tensor('loss_w', (D,), 0) * 10.0).to(DEV)
            (m(x).float() * w).sum().backward()
            torch.cuda.synchronize()
            assert all(b['pending'] == 0 for b in buckets.buckets), [b['pending'] for b in buckets.buckets]
            for k, p in m.named_parameters():
                assert torch.equal(p.grad, ref[k]), f'{prec} recompute={recompute}: {k}'
        finally:
            buckets.remove()
            vtx.set_recompute(False)


# ------------------------------------------------------------------------------------------------ 5. exact arithmetic
@pytest.mark.parametrize('hw', ['0', '3', '16'])
@pytest.mark.parametrize('T,P', [(8, 7), (16, 5)], ids=['L9', 'L17'])
def test_time_cls_packed_kernels_exact(T, P, hw, vtx_opts):
    """attn_fwd_small_kernel<HW, true>, attn_bwd_small_kernel<HW, true>.  B * P = 21 / 15 sequences: not a multiple of the 3
    sequences a tile holds at L = 9, and tiles that straddle two clips (two different cls rows in one tile); H = 5 does not
    divide into groups of 3 or 16.  The case is exact_attn.time_cls_case, run by the layout-aware runners of
    tests/test_gpu_exact_attention.py."""
    import test_gpu_exact_attention as E
    vtx_opts('attn_hw_fwd', hw)
    vtx_opts('attn_hw_bwd', hw)
    c = E.time_cls(3, T, P, 5)
    qkv, out, lse = E.run_fwd(c, BF16)
    E.run_bwd(c, BF16, qkv, out, lse, True)
