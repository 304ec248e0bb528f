"""The exact-fp32 MFMA attention kernels (attn_fwd_f32_kernel, attn_bwd_dq_f32_kernel, attn_bwd_dkv_f32_kernel: the
chunk-streaming kernels of csrc/attn_stream.h with the fp32 tile policy of csrc/attn_f32.hip): fp32 inputs, head_dim 64,
more than 32 tokens, VTX_ATTN_CONTIG and VTX_ATTN_SPACE; option attn_f32 = mfma (default) | valu.

  1. exact arithmetic (tests/exact_attn.py, runners of tests/test_gpu_exact_attention.py) by that module's standard for
     kernels whose probabilities stay in fp32: out equals the exact value bit for bit, lse exactly 0 for one winner and within
     4 fp32 ulps of k ln 2 otherwise; dq, dk, dv and the per-frame cls rows inside the (8 + n) 2^-24 sum|terms| interval of
     exact_attn.value_bounds (the bound counts terms, not their order); sentinel pad columns, rows after the last sequence
     and the lse tail untouched.  Chunks are 64 keys: 33 = one ragged chunk, 128 = two full ones, 129 / 197 / 257 / 385 =
     several + a tail, 1569 = 24 chunks + 33;
  2. a second forward + backward is bit-identical (fixed summation order, no atomics);
  3. random data against the float64 restatement of tests/test_gpu_kernels.py at the joint (8 x 1569 x 12), the 448^2 spatial
     (2 x 4 x 784) and the 224^2 spatial (4 x 8 x 196) shapes with the metric and the fp32 bars that module holds the fp32 VALU
     attention to: TOL[fp32] on out, 1e-4 on lse, 2 TOL[fp32] on dqkv and the per-frame cls rows;
  4. attn_f32=mfma against attn_f32=valu on those shapes within the same bars, and attn_f32=valu as well as attn_f32=mfma
     bit-identical to a build of the parent commit when VTX_PARENT_LIB names one (skipped otherwise);
  5. a joint space-time TimeSformer and a divided one, fp32 forward + backward, mfma against valu within the fp32 model bars
     of tests/helpers.py;
  6. one bf16 case of each existing route (<= 32 tokens, 197, 1569, attn_valu=1) is bit-identical with attn_f32 at either value.
"""
import pytest
import torch

import test_gpu_exact_attention as E
from helpers import TOL_F32, check, l2err, report
from test_gpu_kernels import TOL, _attn_ref, dev, q, rnd
from test_gpu_long_attention import _ref_lse, assert_parent_bit_for_bit

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
BF16, F32 = torch.bfloat16, torch.float32
LSE_BAR = 1e-4                                   # tests/test_gpu_kernels.py: the lse bar of the attention kernels


@pytest.fixture
def attn_f32():
    """set(value) -> vtx.set_option('attn_f32', value); back to the default afterwards (tests/conftest.py's vtx_opts does
    not know this switch)."""
    import vtx
    try:
        yield lambda v: vtx.set_option('attn_f32', v)
    finally:
        vtx.set_option('attn_f32', 'mfma')


def run_f32(c):
    assert c.hd == 64 and c.L > 32                                      # attn.hip: attn_route
    qkv, out, lse = E.run_fwd(c, F32)
    res = (out, lse)
    if c.bwd:
        res += E.run_bwd(c, F32, qkv, out, lse, False)                  # exact=False: the interval of fp32 probabilities
    return res


def _bits(t):
    return t.view(torch.int16) if t.dtype == BF16 else t.view(torch.int32)


# ------------------------------------------------------------------------------------------------ 1. exact
@pytest.mark.parametrize('S,L,H', [(3, 33, 2), (3, 128, 2), (3, 129, 2), (3, 197, 3), (2, 257, 2), (3, 385, 3), (1, 1569, 2)])
def test_f32_contig_exact(S, L, H, attn_f32):
    attn_f32('mfma')
    run_f32(E.contig(S, L, H))


@pytest.mark.parametrize('B,T,P,H', [(2, 3, 196, 2), (2, 3, 300, 2), (1, 2, 784, 2)])
def test_f32_space_exact(B, T, P, H, attn_f32):
    attn_f32('mfma')
    run_f32(E.space(B, T, P, H))


# ------------------------------------------------------------------------------------------------ 2. determinism
def test_f32_is_bit_reproducible(attn_f32):
    attn_f32('mfma')
    c = E.contig(1, 1569, 2)
    first = run_f32(c)
    again = run_f32(c)
    for a, b in zip(first, again):
        if a is not None:
            assert torch.equal(_bits(a), _bits(b)), 'second run differs'


# ------------------------------------------------------------------------------------------------ 3. / 4. random data
def _run_contig(qkv, do, S, L, H, dtype=F32):
    from vtx import ops
    from vtx._lib import ATTN_CONTIG
    hd, D = 64, H * 64
    o = torch.full((S, L, D), float('nan'), dtype=dtype, device=DEV)
    lse = torch.full((S * H * L,), float('nan'), device=DEV)
    ops.attn_fwd(qkv, o, lse, ATTN_CONTIG, S, L, H, hd, hd ** -0.5)
    dqkv = torch.full((S, L, 3 * D), float('nan'), dtype=dtype, device=DEV)
    ops.attn_bwd(qkv, o, lse, do, dqkv, ATTN_CONTIG, S, L, H, hd, hd ** -0.5)
    torch.cuda.synchronize()
    return o, lse, dqkv


def _run_space(qkv, do, B, T, P, H, dtype=F32):
    """(out, lse, dqkv before cls_qkv_reduce, per-frame cls rows)"""
    from vtx import ops
    from vtx._lib import ATTN_SPACE
    hd, D, N, L = 64, H * 64, P * T, P + 1
    o = torch.full((B * N + B * T, D), float('nan'), dtype=dtype, device=DEV)
    lse = torch.full((B * T * H * L,), float('nan'), device=DEV)
    ops.attn_fwd(qkv, o, lse, ATTN_SPACE, B * T, L, H, hd, hd ** -0.5, B, T, P)
    dqkv = torch.zeros(B, 1 + N, 3 * D, dtype=dtype, device=DEV)
    dcls = torch.full((B * T, 3 * D), float('nan'), dtype=dtype, device=DEV)
    ops.attn_bwd(qkv, o, lse, do, dqkv, ATTN_SPACE, B * T, L, H, hd, hd ** -0.5, B, T, P, dqkv_cls=dcls)
    torch.cuda.synchronize()
    return o, lse, dqkv, dcls


def _contig_inputs(S, L, H):
    D = H * 64
    return rnd(S, L, 3 * D, seed=L) * 1.5, rnd(S, L, D, seed=L + 1)


def _space_inputs(B, T, P, H):
    D, N = H * 64, P * T
    return rnd(B, 1 + N, 3 * D, seed=1) * 1.5, rnd(B, N, D, seed=2), rnd(B * T, D, seed=3)


def test_f32_contig_vs_float64_and_valu_at_joint_scale(attn_f32):
    """8 clips of joint space-time attention.  The float64 reference runs on the device, one sequence at a time (a
    [12, 1569, 1569] float64 score matrix is 236 MB)."""
    S, L, H, hd = 8, 1569, 12, 64
    scale = hd ** -0.5
    qkv, do = _contig_inputs(S, L, H)
    qq = q(qkv, F32).to(DEV).requires_grad_(True)
    dd = q(do, F32).to(DEV)
    refs, lses = [], []
    for s in range(S):
        r, _ = _attn_ref(qq[s:s + 1], H)
        r.backward(dd[s:s + 1])
        refs.append(r.detach())
        lses.append(_ref_lse(qq[s:s + 1].detach(), H, hd, scale))
    ref, lse_ref = torch.cat(refs).cpu(), torch.cat(lses).cpu()
    qd, dod = dev(qkv, F32), dev(do, F32)
    attn_f32('mfma')
    new = _run_contig(qd, dod, S, L, H)
    attn_f32('valu')
    old = _run_contig(qd, dod, S, L, H)
    name = f'contig {S}x{H}x{L}'
    for tag, (o, lse, dqkv) in (('mfma', new), ('valu', old)):
        check(f'attn f32 {tag} fwd {name} vs f64', o.cpu(), ref, TOL[F32])
        check(f'attn f32 {tag} lse {name} vs f64', lse.cpu().reshape(S, H, L), lse_ref, LSE_BAR)
        check(f'attn f32 {tag} bwd {name} vs f64', dqkv.cpu(), qq.grad.cpu(), 2 * TOL[F32])
    for what, a, b, bar in zip(('out', 'lse', 'dqkv'), new, old, (TOL[F32], LSE_BAR, 2 * TOL[F32])):
        check(f'attn f32 mfma vs valu {what} {name}', a.cpu(), b.cpu(), bar)


@pytest.mark.parametrize('B,T,P', [(2, 4, 784), (4, 8, 196)])
def test_f32_space_vs_float64_and_valu(B, T, P, attn_f32):
    from vtx import ops
    H, hd = 12, 64
    L, N, D, scale = P + 1, P * T, H * hd, hd ** -0.5
    qkv, do_tok_, do_cls_ = _space_inputs(B, T, P, H)
    do_tok, do_cls = q(do_tok_, F32).to(DEV), q(do_cls_, F32).to(DEV)
    qq = q(qkv, F32).to(DEV).requires_grad_(True)
    tok = qq[:, 1:].reshape(B, P, T, 3 * D).permute(0, 2, 1, 3).reshape(B * T, P, 3 * D)
    cls = qq[:, :1].expand(B, T, 3 * D).reshape(B * T, 1, 3 * D)
    seqs = torch.cat([cls, tok], 1)                                     # [(b t), 1+P, 3D]
    ref, _ = _attn_ref(seqs, H)
    ref_tok = ref[:, 1:].reshape(B, T, P, D).permute(0, 2, 1, 3).reshape(B, N, D)
    ref_cls = ref[:, 0]
    ((ref_tok * do_tok).sum() + (ref_cls * do_cls).sum()).backward()
    lse_ref = _ref_lse(seqs.detach(), H, hd, scale).cpu()
    # per-frame cls rows: d(loss)/d(the cls copy of frame (b, t))
    seqs2 = seqs.detach().clone().requires_grad_(True)
    r2, _ = _attn_ref(seqs2, H)
    r2_tok = r2[:, 1:].reshape(B, T, P, D).permute(0, 2, 1, 3).reshape(B, N, D)
    ((r2_tok * do_tok).sum() + (r2[:, 0] * do_cls).sum()).backward()
    qd = dev(qkv, F32)
    dout = torch.cat([do_tok.reshape(B * N, D), do_cls], 0).to(F32).contiguous()
    attn_f32('mfma')
    new = _run_space(qd, dout, B, T, P, H)
    attn_f32('valu')
    old = _run_space(qd, dout, B, T, P, H)
    name = f'space {B}x{T}x{P} H={H}'
    bars = (TOL[F32], LSE_BAR, 2 * TOL[F32], 2 * TOL[F32])
    for what, a, b, bar in zip(('out', 'lse', 'dqkv tokens', 'dqkv_cls'), new, old, bars):
        check(f'attn f32 mfma vs valu {what} {name}', a.cpu(), b.cpu(), bar)
    for tag, (o, lse, dqkv, dcls) in (('mfma', new), ('valu', old)):
        check(f'attn f32 {tag} fwd tokens {name} vs f64', o[:B * N].cpu().reshape(B, N, D), ref_tok.detach().cpu(), TOL[F32])
        check(f'attn f32 {tag} fwd cls {name} vs f64', o[B * N:].cpu(), ref_cls.detach().cpu(), TOL[F32])
        check(f'attn f32 {tag} lse {name} vs f64', lse.cpu().reshape(B * T, H, L), lse_ref, LSE_BAR)
        check(f'attn f32 {tag} bwd cls rows {name} vs f64', dcls.cpu(), seqs2.grad[:, 0].cpu(), 2 * TOL[F32])
        full = dqkv.clone()
        ops.cls_qkv_reduce(dcls, full, B, T, 3 * D, 1 + N)
        check(f'attn f32 {tag} bwd {name} vs f64', full.cpu(), qq.grad.cpu(), 2 * TOL[F32])


PARENT_CONTIG = [(2, 197, 3), (2, 1569, 3)]
PARENT_SPACE = [(2, 2, 196, 3), (1, 2, 784, 3)]


def test_f32_valu_is_the_parent_bit_for_bit(attn_f32, tmp_path):
    """attn_f32=valu against a libvtx.so built from the parent commit, named by VTX_PARENT_LIB (both builds are told
    attn_f32=valu: the parent's default is the MFMA route as well)."""
    spec = dict(dtype='float32', options={'attn_f32': 'valu'}, contig=PARENT_CONTIG, space=PARENT_SPACE)
    try:
        assert_parent_bit_for_bit(spec, tmp_path, 'attn_f32=valu')
    finally:
        attn_f32('mfma')


def test_f32_mfma_is_the_parent_bit_for_bit(attn_f32, tmp_path):
    """The default fp32 route (attn_f32=mfma) against a libvtx.so built from the parent commit, named by VTX_PARENT_LIB:
    one ragged chunk (33), full chunks only (128), several + a tail (197), 24 chunks + a tail and an idle wave (1569), and the
    cls row of the space layout."""
    spec = dict(dtype='float32', options={'attn_f32': 'mfma'}, contig=[(2, 33, 3), (2, 128, 3), (2, 197, 3), (2, 1569, 3)],
                space=[(1, 2, 784, 3), (2, 2, 196, 3)])
    try:
        assert_parent_bit_for_bit(spec, tmp_path, 'attn_f32=mfma')
    finally:
        attn_f32('mfma')


# ------------------------------------------------------------------------------------------------ 5. models
@pytest.mark.parametrize('at,kw,frames', [('joint_space_time', dict(img_size=64, patch_size=8), 8),         # L = 1 + 64 * 8 = 513
                                          ('divided_space_time', dict(img_size=160, patch_size=8), 2)])    # P = 400
def test_timesformer_fp32_mfma_against_valu_attention(at, kw, frames, attn_f32):
    import vtx
    import video_transformer as V
    from model_common import _build, _train_step
    from oracle import synth
    vtx.set_precision('fp32')
    try:
        cfg = dict(embed_dims=128, num_heads=2, num_transformer_layers=2, **kw)
        x = synth.synth_clip(2, frames, 3, kw['img_size'], kw['img_size'], seed=2)
        res = {}
        for mode in ('mfma', 'valu'):
            attn_f32(mode)
            m, _ = _build(V.TimeSformer, 3, num_frames=frames, attention_type=at, **cfg)
            y, grads = _train_step(m, x, 11, 128)
            res[mode] = (y.detach().float().cpu(), {k: v.detach().float().cpu() for k, v in grads.items()})
    finally:
        vtx.set_precision('auto')
    check(f'tsf {at} fp32 mfma attention vs valu: out', res['mfma'][0], res['valu'][0], TOL_F32)
    assert set(res['mfma'][1]) == set(res['valu'][1]) and res['mfma'][1]
    worst = 0.0
    for k, g in res['mfma'][1].items():
        e = l2err(g, res['valu'][1][k])
        worst = max(worst, e)
        assert e <= TOL_F32, f'{at} grad {k}: rel L2 {e:.3e} > {TOL_F32:g}'
    report(f'ok   tsf {at} fp32 mfma attention vs valu: {len(res["mfma"][1])} gradients, worst rel L2 {worst:.3e} (tol {TOL_F32:g})')


# ------------------------------------------------------------------------------------------------ 6. bf16 untouched
@pytest.mark.parametrize('route', ['short', '197', '1569', 'valu'])
def test_bf16_routes_ignore_attn_f32(route, attn_f32, vtx_opts):
    S, L = {'short': (37, 8), '197': (3, 197), '1569': (1, 1569), 'valu': (3, 197)}[route]
    H = 3
    if route == 'valu':
        vtx_opts('attn_valu', '1')
    qkv, do = _contig_inputs(S, L, H)
    qd, dod = dev(qkv, BF16), dev(do, BF16)
    attn_f32('mfma')
    a = _run_contig(qd, dod, S, L, H, BF16)
    attn_f32('valu')
    b = _run_contig(qd, dod, S, L, H, BF16)
    assert all(torch.isfinite(t.float()).all() for t in a)
    for x, y in zip(a, b):
        assert torch.equal(_bits(x), _bits(y)), f'bf16 {route}: attn_f32 changes the result'
