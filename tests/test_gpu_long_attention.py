"""The bf16 MFMA attention kernels for more than 256 tokens (attn_fwd_long_kernel, attn_bwd_dq_long_kernel,
attn_bwd_dkv_long_kernel: the chunk-streaming kernels of csrc/attn_stream.h with the bf16 tile policy of csrc/attn_long.hip),
VTX_ATTN_CONTIG and VTX_ATTN_SPACE.

  1. exact arithmetic (tests/exact_attn.py, runners of tests/test_gpu_exact_attention.py): every output equals RNE(exact) --
     the MFMA standard of that module, which its own _mfma_path only grants up to 256 tokens; lse exactly 0 for one winner,
     within 4 fp32 ulps of k ln 2 otherwise; sentinel pad columns, rows after the last sequence and the lse tail untouched.
     257 = one key past a chunk pair, 385 = 3 chunks + 1, 1569 = 12 chunks + 33.  A chunk that holds only losers for a query
     accumulates integer V sums and is wiped by a rescale of exactly exp2(<= -369) = 0, so online softmax is covered exactly;
  2. a second backward run is bit-identical (fixed summation order, no atomics);
  3. random data against the float64 restatement of tests/test_gpu_kernels.py at the joint (8 x 1569 x 12) and the 448^2
     spatial (2 x 4 x 784, 12 heads) shapes, with the metric and bars that module holds the <= 256-token MFMA kernels to:
     TOL[bf16] on out, 1e-4 on lse, 2 TOL[bf16] on dqkv and the per-frame cls rows;
  4. attn_long=1 against attn_long=0 (two implementations of one op: 1e-2 / 1e-4 / 2e-2), and attn_long=0 bit-identical to
     attn_valu=1 (the fallback is the old path); attn_long=1 bit-identical to a build of the parent commit when VTX_PARENT_LIB
     names one (skipped otherwise): out, lse, dqkv and the per-frame cls rows;
  5. a joint space-time TimeSformer and a divided one whose spatial sequence has 401 tokens, bf16 forward + backward,
     attn_long=1 against attn_long=0 within the bf16 model bars of tests/helpers.py.
"""
import json
import os
import subprocess
import sys

import pytest
import torch

import exact_attn as A
import test_gpu_exact_attention as E
from helpers import ROOT, TOL_BF16, TOL_BF16_GRAD, check, l2err, report
from test_gpu_kernels import TOL, _attn_ref, dev, q, rnd

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
BF16 = torch.bfloat16


@pytest.fixture
def attn_long():
    """set(value) -> vtx.set_option('attn_long', value); back to the default afterwards (tests/conftest.py's vtx_opts does
    not know this switch)."""
    import vtx
    try:
        yield lambda v: vtx.set_option('attn_long', v)
    finally:
        vtx.set_option('attn_long', '1')


def _long_mfma_path(c, dtype):
    """Whether vtx_attn_* takes the kernels of attn_long.hip at default options (attn.hip: attn_route)."""
    return dtype == BF16 and c.hd == 64 and c.L > 256


def run_long(c):
    assert _long_mfma_path(c, BF16)
    qkv, out, lse = E.run_fwd(c, BF16)
    res = (out, lse)
    if c.bwd:
        res += E.run_bwd(c, BF16, qkv, out, lse, True)           # exact=True: RNE equality, the MFMA standard
    return res


def _bits(t):
    return t.view(torch.int16) if t.dtype == BF16 else t.view(torch.int32)


# ------------------------------------------------------------------------------------------------ 1. exact
@pytest.mark.parametrize('S,L,H', [(2, 257, 2), (2, 300, 2), (3, 385, 3), (1, 1569, 2)])
def test_long_contig_exact(S, L, H):
    run_long(E.contig(S, L, H))


def test_long_contig_forward_round_exact():
    run_long(E.contig(2, 1569, 12, 'round', False))


@pytest.mark.parametrize('B,T,P,H', [(2, 3, 300, 2), (1, 2, 784, 2)])
def test_long_space_exact(B, T, P, H):
    run_long(E.space(B, T, P, H))


# ------------------------------------------------------------------------------------------------ 2. determinism
def test_long_backward_is_bit_reproducible():
    c = E.contig(1, 1569, 2)
    first = run_long(c)
    again = run_long(c)
    for a, b in zip(first, again):
        if a is not None:
            assert torch.equal(_bits(a), _bits(b)), 'second run differs'


# ------------------------------------------------------------------------------------------------ 3. float64, random data
def _ref_lse(seqs, H, hd, scale):                                       # [S, L, 3D] float64 -> [S, H, L]
    S, L = seqs.shape[:2]
    t = seqs.reshape(S, L, 3, H, hd)
    qh, kh = t[:, :, 0].permute(0, 2, 1, 3), t[:, :, 1].permute(0, 2, 1, 3)
    return torch.logsumexp(qh @ kh.transpose(-1, -2) * scale, dim=-1)


def test_long_contig_vs_float64_at_joint_scale():
    """8 clips of joint space-time attention.  The float64 reference runs on the device, one sequence at a time (a
    [12, 1569, 1569] float64 score matrix is 236 MB)."""
    from vtx import ops
    from vtx._lib import ATTN_CONTIG
    S, L, H, hd = 8, 1569, 12, 64
    D, scale = H * hd, hd ** -0.5
    qkv = rnd(S, L, 3 * D, seed=L) * 1.5
    do = rnd(S, L, D, seed=L + 1)
    qq = q(qkv, BF16).to(DEV).requires_grad_(True)
    dd = q(do, BF16).to(DEV)
    refs, lses = [], []
    for s in range(S):
        r, _ = _attn_ref(qq[s:s + 1], H)
        r.backward(dd[s:s + 1])
        refs.append(r.detach())
        lses.append(_ref_lse(qq[s:s + 1].detach(), H, hd, scale))
    ref, lse_ref = torch.cat(refs), torch.cat(lses)
    qd = dev(qkv, BF16)
    o = torch.full((S, L, D), float('nan'), dtype=BF16, device=DEV)
    lse = torch.full((S * H * L,), float('nan'), device=DEV)
    ops.attn_fwd(qd, o, lse, ATTN_CONTIG, S, L, H, hd, scale)
    dqkv = torch.full((S, L, 3 * D), float('nan'), dtype=BF16, device=DEV)
    ops.attn_bwd(qd, o, lse, dev(do, BF16), dqkv, ATTN_CONTIG, S, L, H, hd, scale)
    check(f'attn long fwd contig {S}x{H}x{L} vs f64', o.float().cpu(), ref.cpu(), TOL[BF16])
    check(f'attn long lse contig {S}x{H}x{L} vs f64', lse.cpu().reshape(S, H, L), lse_ref.cpu(), 1e-4)
    check(f'attn long bwd contig {S}x{H}x{L} vs f64', dqkv.float().cpu(), qq.grad.cpu(), 2 * TOL[BF16])


def test_long_space_vs_float64_at_448_scale():
    from vtx import ops
    from vtx._lib import ATTN_SPACE
    B, T, P, H, hd = 2, 4, 784, 12, 64
    L, N, D, scale = P + 1, P * T, H * hd, hd ** -0.5
    qkv = rnd(B, 1 + N, 3 * D, seed=1) * 1.5
    do_tok = q(rnd(B, N, D, seed=2), BF16).to(DEV)
    do_cls = q(rnd(B * T, D, seed=3), BF16).to(DEV)
    qq = q(qkv, BF16).to(DEV).requires_grad_(True)
    tok = qq[:, 1:].reshape(B, P, T, 3 * D).permute(0, 2, 1, 3).reshape(B * T, P, 3 * D)
    cls = qq[:, :1].expand(B, T, 3 * D).reshape(B * T, 1, 3 * D)
    seqs = torch.cat([cls, tok], 1)                                     # [(b t), 1+P, 3D]
    ref, _ = _attn_ref(seqs, H)
    ref_tok = ref[:, 1:].reshape(B, T, P, D).permute(0, 2, 1, 3).reshape(B, N, D)
    ref_cls = ref[:, 0]
    ((ref_tok * do_tok).sum() + (ref_cls * do_cls).sum()).backward()
    lse_ref = _ref_lse(seqs.detach(), H, hd, scale)
    qd = dev(qkv, BF16)
    o = torch.full((B * N + B * T, D), float('nan'), dtype=BF16, device=DEV)
    lse = torch.full((B * T * H * L,), float('nan'), device=DEV)
    ops.attn_fwd(qd, o, lse, ATTN_SPACE, B * T, L, H, hd, scale, B, T, P)
    name = f'{B}x{T}x{P} H={H} vs f64'
    check(f'attn long fwd space tokens {name}', o[:B * N].float().cpu().reshape(B, N, D), ref_tok.detach().cpu(), TOL[BF16])
    check(f'attn long fwd space cls {name}', o[B * N:].float().cpu(), ref_cls.detach().cpu(), TOL[BF16])
    check(f'attn long lse space {name}', lse.cpu().reshape(B * T, H, L), lse_ref.cpu(), 1e-4)
    dout = torch.cat([do_tok.reshape(B * N, D), do_cls], 0).to(BF16)
    dqkv = torch.zeros(B, 1 + N, 3 * D, dtype=BF16, device=DEV)
    dqkv_cls = torch.full((B * T, 3 * D), float('nan'), dtype=BF16, device=DEV)
    ops.attn_bwd(qd, o, lse, dout, dqkv, ATTN_SPACE, B * T, L, H, hd, scale, B, T, P, dqkv_cls=dqkv_cls)
    # per-frame cls rows: d(loss)/d(the cls copy of frame (b, t))
    seqs2 = seqs.detach().clone().requires_grad_(True)
    r2, _ = _attn_ref(seqs2, H)
    r2_tok = r2[:, 1:].reshape(B, T, P, D).permute(0, 2, 1, 3).reshape(B, N, D)
    ((r2_tok * do_tok).sum() + (r2[:, 0] * do_cls).sum()).backward()
    check(f'attn long bwd space cls rows {name}', dqkv_cls.float().cpu(), seqs2.grad[:, 0].cpu(), 2 * TOL[BF16])
    ops.cls_qkv_reduce(dqkv_cls, dqkv, B, T, 3 * D, 1 + N)
    check(f'attn long bwd space {name}', dqkv.float().cpu(), qq.grad.cpu(), 2 * TOL[BF16])


# ------------------------------------------------------------------------------------------------ 4. long vs VALU
def _run_contig(qkv, do, S, L, H, dtype=BF16):
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


def _run_space(qkv, do, B, T, P, H, dtype=BF16):
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


@pytest.mark.parametrize('shape', [('contig', 3, 385), ('contig', 2, 1569), ('space', 2, 2, 300), ('space', 1, 2, 784)])
def test_long_matches_valu_and_fallback_is_the_old_path(shape, attn_long, vtx_opts):
    H, D = 3, 3 * 64
    if shape[0] == 'contig':
        _, S, L = shape
        qkv = dev(rnd(S, L, 3 * D, seed=5) * 1.5, BF16)
        do = dev(rnd(S, L, D, seed=6), BF16)
        run = lambda: _run_contig(qkv, do, S, L, H)                      # noqa: E731
    else:
        _, B, T, P = shape
        qkv = dev(rnd(B, 1 + P * T, 3 * D, seed=5) * 1.5, BF16)
        do = dev(rnd(B * P * T + B * T, D, seed=6), BF16)
        run = lambda: _run_space(qkv, do, B, T, P, H)                    # noqa: E731
    new = run()
    attn_long('0')
    old = run()
    attn_long('1')
    vtx_opts('attn_valu', '1')
    valu = run()
    name = ' '.join(str(x) for x in shape)
    assert all(torch.isfinite(t.float()).all() for t in new)
    for a, b in zip(old, valu):
        assert torch.equal(_bits(a), _bits(b)), f'{name}: attn_long=0 differs from attn_valu=1'
    bars = (1e-2, 1e-4, 2e-2, 2e-2)
    for what, a, b, bar in zip(('out', 'lse', 'dqkv', 'dqkv_cls'), new, old, bars):
        check(f'attn long vs valu {what} {name}', a.float().cpu(), b.float().cpu(), bar)


# ---- against a build of the parent commit ----
# What a library computes for a list of shapes: {case: (out, lse, dqkv[, dqkv_cls])} on the CPU.  spec = {'dtype': name of a
# torch dtype, 'options': {option: value} set first, 'contig': [(S, L, H)], 'space': [(B, T, P, H)]}.
def parent_cases(spec):
    import vtx
    dtype = getattr(torch, spec['dtype'])
    for k, v in spec['options'].items():
        vtx.set_option(k, v)
    res = {}
    for S, L, H in spec['contig']:
        qkv, do = rnd(S, L, 3 * H * 64, seed=L) * 1.5, rnd(S, L, H * 64, seed=L + 1)
        res[f'contig {S} {L} {H}'] = [t.cpu() for t in _run_contig(dev(qkv, dtype), dev(do, dtype), S, L, H, dtype)]
    for B, T, P, H in spec['space']:
        qkv, do = rnd(B, 1 + P * T, 3 * H * 64, seed=1) * 1.5, rnd(B * P * T + B * T, H * 64, seed=2)
        res[f'space {B} {T} {P} {H}'] = [t.cpu() for t in _run_space(dev(qkv, dtype), dev(do, dtype), B, T, P, H, dtype)]
    return res


# the same in a child process that loads the library VTX_LIB names (a process loads one library)
_PARENT_JOB = r'''
import importlib, json, sys, torch
sys.path[:0] = sys.argv[1:4]
cases = getattr(importlib.import_module(sys.argv[5]), sys.argv[6])
torch.save(cases(json.loads(sys.argv[7])), sys.argv[4])
'''


def parent_build_cases(cases, spec, tmp_path):
    """cases(spec) -- a module-level function of a test module, {case: [CPU tensors]} -- as the library named by VTX_PARENT_LIB
    (built from the parent commit) computes it in a child process; skipped when VTX_PARENT_LIB names no file.  Returns that
    dict and the library's file name; this process is asserted to run another library."""
    import vtx
    parent = os.environ.get('VTX_PARENT_LIB', '')
    if not parent or not os.path.isfile(parent):
        print('skipped: VTX_PARENT_LIB does not name a library built from the parent commit')
        pytest.skip('VTX_PARENT_LIB does not name a library built from the parent commit')
    out = str(tmp_path / 'parent.pt')
    env = dict(os.environ, VTX_LIB=os.path.abspath(parent))
    for k in ('VTX_ATTN_F32', 'VTX_ATTN_LONG', 'VTX_ATTN_VALU', 'VTX_LN_ROWS', 'VTX_GEMM_TN'):
        env.pop(k, None)
    subprocess.run([sys.executable, '-c', _PARENT_JOB, ROOT, os.path.join(ROOT, 'videotransformer-pytorch_amd'),
                    os.path.join(ROOT, 'tests'), out, cases.__module__, cases.__name__, json.dumps(spec)], check=True, env=env, timeout=600)
    want = torch.load(out)
    assert os.path.realpath(vtx.load()._name) != os.path.realpath(parent), 'this process runs the parent library itself'
    return want, os.path.basename(parent)


def assert_parent_bit_for_bit(spec, tmp_path, what):
    """Every tensor of parent_cases(spec) from this build equals, bit for bit, what the library named by VTX_PARENT_LIB (built
    from the parent commit) computes; skipped when VTX_PARENT_LIB names no file."""
    want, parent = parent_build_cases(parent_cases, spec, tmp_path)
    got = parent_cases(spec)
    assert sorted(got) == sorted(want) and len(got) == len(spec['contig']) + len(spec['space'])
    names = ('out', 'lse', 'dqkv', 'dqkv_cls')
    for case in got:
        assert len(got[case]) == len(want[case]) == (4 if case.startswith('space') else 3)
        for name, a, b in zip(names, got[case], want[case]):
            assert a.dtype == b.dtype and a.shape == b.shape
            assert torch.isfinite(a.float()).any(), f'{case}: {name} was never written'
            assert torch.equal(_bits(a), _bits(b)), f'{case}: {name} of {what} differs from the parent'
    report(f'ok   {what} bit-identical to {parent} on {len(got)} shapes: ' + ', '.join(got))


def test_long_is_the_parent_bit_for_bit(attn_long, tmp_path):
    """The default bf16 route (attn_long=1) against a libvtx.so built from the parent commit, named by VTX_PARENT_LIB:
    one ragged chunk past two full ones (257), full chunks + one key (385), 12 chunks + a tail and an idle wave (1569), and
    the cls row of the space layout."""
    spec = dict(dtype='bfloat16', options={'attn_long': '1'}, contig=[(2, 257, 3), (2, 385, 3), (2, 1569, 3)], space=[(1, 2, 784, 3)])
    try:
        assert_parent_bit_for_bit(spec, tmp_path, 'attn_long=1')
    finally:
        attn_long('1')


# ------------------------------------------------------------------------------------------------ 5. models
@pytest.mark.parametrize('at,kw,frames', [('joint_space_time', dict(img_size=64, patch_size=8), 8),         # L = 1 + 64 * 8 = 513
                                          ('divided_space_time', dict(img_size=160, patch_size=8), 2)])    # P = 400
def test_timesformer_long_sequences_against_valu_attention(at, kw, frames, attn_long):
    import vtx
    import video_transformer as V
    from model_common import _build, _train_step
    from oracle import synth
    vtx.set_precision('bf16')
    try:
        cfg = dict(embed_dims=128, num_heads=2, num_transformer_layers=2, **kw)
        x = synth.synth_clip(2, frames, 3, kw['img_size'], kw['img_size'], seed=2)
        res = {}
        for mode in ('1', '0'):
            attn_long(mode)
            m, _ = _build(V.TimeSformer, 3, num_frames=frames, attention_type=at, **cfg)
            y, grads = _train_step(m, x, 11, 128)
            res[mode] = (y.detach().float().cpu(), {k: v.detach().float().cpu() for k, v in grads.items()})
    finally:
        vtx.set_precision('auto')
    check(f'tsf {at} long attention vs valu: out', res['1'][0], res['0'][0], TOL_BF16)
    assert set(res['1'][1]) == set(res['0'][1]) and res['1'][1]
    worst = 0.0
    for k, g in res['1'][1].items():
        e = l2err(g, res['0'][1][k])
        worst = max(worst, e)
        assert e <= TOL_BF16_GRAD, f'{at} grad {k}: rel L2 {e:.3e} > {TOL_BF16_GRAD:g}'
    report(f'ok   tsf {at} long attention vs valu: {len(res["1"][1])} gradients, worst rel L2 {worst:.3e} (tol {TOL_BF16_GRAD:g})')
