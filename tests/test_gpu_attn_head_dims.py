"""Self-attention at head_dim 32, 96 and 128 (vtx_attn_fwd / vtx_attn_bwd): the VALU kernels of csrc/attn.hip instantiated
for those head dims (fp32; bf16 up to 32 tokens; `probs`; attn_hd=valu) and the chunk-streaming MFMA kernels of csrc/attn_hd.hip
(bf16, more than 32 tokens; option attn_hd = mfma, the default).  Chunks there hold 64 keys; a workgroup owns 128 queries, a
wave a 32-row tile.

  1. every layout against the float64 restatement of tests/test_gpu_kernels.py, fed the operands as the compute dtype holds
     them: TOL[dtype] on out, 1e-4 on lse, 2 TOL[dtype] on dqkv and on the per-sequence cls rows -- the bars the head_dim-64
     kernels are held to, imported.  Buffers start as the NaN sentinel of tests/exact.py with 8 pad columns per row (ld_qkv,
     ld_out, ld_dout, ld_dqkv), two rows after the last sequence and a tail on lse: none of them may change.  L = 33, 65, 129,
     257: one key past a 32-row tile, a 64-row chunk, a chunk pair (and a workgroup's 128 rows), two chunk pairs;
  2. exact arithmetic (tests/exact_attn.py, runners of tests/test_gpu_exact_attention.py) for the MFMA route: every output
     equals RNE(exact), lse exactly 0 for one winner and within 4 fp32 ulps of k ln 2 otherwise;
  3. a second run is bit-identical;
  4. attn_hd=mfma against attn_hd=valu (two implementations of one op: the bars of tests/test_gpu_long_attention.py section
     4), and head_dim 64 bit-identical under both values;
  5. TimeSformer (divided space-time, joint space-time), ViViT fact_encoder and a space-then-time container at head_dim 32,
     96 and 128 against the CPU oracle, forward + backward, fp32 and bf16, with the model bars of tests/helpers.py;
     get_last_selfattention; the exact residual stream;
  6. head_dim 64 against a build of the parent commit, bit for bit, one shape per route (VTX_PARENT_LIB; skipped otherwise).
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import exact as X
import exact_attn as A
import test_gpu_exact_attention as E
from helpers import TOL_BF16, TOL_BF16_GRAD, TOL_F32, check, l2err, relerr, report
from oracle import synth, vt_oracle as O
from oracle.synth import synth_tensor
from test_gpu_cls_order import LSE_BAR
from test_gpu_kernels import TOL, _attn_ref, dev, q, rnd
from test_gpu_long_attention import _bits, _ref_lse, assert_parent_bit_for_bit

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
BF16, F32 = torch.bfloat16, torch.float32
PAD = E.PAD
HDS = [32, 96, 128]
IDS = {BF16: 'bf16', F32: 'fp32'}


@pytest.fixture
def attn_hd():
    """set(value) -> vtx.set_option('attn_hd', value); back to the default afterwards (tests/conftest.py's vtx_opts does
    not know this switch)."""
    import vtx
    try:
        yield lambda v: vtx.set_option('attn_hd', v)
    finally:
        vtx.set_option('attn_hd', 'mfma')


@pytest.fixture(autouse=True)
def _defaults():
    import vtx
    yield
    vtx.set_precision('auto')
    vtx.set_stream('bf16')


# ------------------------------------------------------------------------------------------------ 1. float64
def _geometry(layout, dims):
    """(S, L, B, T, P, rows of qkv, rows of out, in-rows [S, L], out-rows [S, L], sequences per shared cls row)"""
    if layout == 'contig':
        S, L = dims
        r = np.arange(S * L).reshape(S, L)
        return S, L, 0, 0, 0, S * L, S * L, r, r, 0
    B, T, P = dims
    rin, rout = A.layout_rows(layout, B, T, P)
    S, L = rin.shape
    grp = {'space': T, 'time_cls': P, 'space_nocls': 0}[layout]
    return S, L, B, T, P, B * (1 + P * T), B * P * T + (S if grp else 0), rin, rout, grp


def _ramp_qkv(S, L, H, hd, seed):
    """contig qkv [S L, 3D] whose scaled scores rise by about 8 along the keys: with u = ones(hd) / sqrt(hd), q_i = u + noise / 4
    and k_j = (j / L) (8 / scale) u + noise / 4, so the running maximum of the online softmax moves at every 8-key chunk and
    across every 64-key tile; v is random."""
    D = H * hd
    noise = rnd(S * L, 3 * D, seed=seed)
    u = hd ** -0.5
    j = (torch.arange(S * L) % L).float()[:, None] / L
    qkv = noise.clone()
    qkv[:, :D] = u + 0.25 * noise[:, :D]
    qkv[:, D:2 * D] = j * (8.0 * hd ** 0.5) * u + 0.25 * noise[:, D:2 * D]
    return qkv


@functools.lru_cache(maxsize=None)
def _reference(layout, dims, H, hd, dtype, operands='random'):
    """Inputs (float32 CPU) and the float64 results on the operands as `dtype` holds them: out [out rows, D], lse [S, H, L],
    dqkv [qkv rows, 3D] (the shared cls rows summed over their sequences), the per-sequence cls rows [S, 3D].  operands: 'random'
    (dense normal data) or 'ramp' (_ramp_qkv; contig only)."""
    S, L, B, T, P, rows, orows, rin, rout, grp = _geometry(layout, dims)
    D = H * hd
    if operands == 'ramp':
        assert layout == 'contig'
        qkv = _ramp_qkv(S, L, H, hd, L + hd)
    else:
        assert operands == 'random'
        qkv = rnd(rows, 3 * D, seed=L + hd) * 1.5
    do = rnd(orows, D, seed=L + hd + 1)
    base = q(qkv, dtype).requires_grad_(True)
    seqs = base[torch.from_numpy(rin)]                                  # [S, L, 3D]
    seqs.retain_grad()
    ref, _ = _attn_ref(seqs, H)
    (ref * q(do, dtype)[torch.from_numpy(rout)]).sum().backward()
    out = torch.zeros(orows, D, dtype=torch.float64)
    out[torch.from_numpy(rout.reshape(-1))] = ref.detach().reshape(S * L, D)
    lse = _ref_lse(seqs.detach(), H, hd, hd ** -0.5)
    return qkv, do, out, lse, base.grad, seqs.grad[:, 0].clone()


def _padded(a, dtype, extra_rows=0):
    """[rows, n] CPU -> device [rows + extra_rows, n + PAD], the sentinel (a NaN) everywhere else"""
    t = X.guarded((a.shape[0] + extra_rows, a.shape[1]), dtype, DEV, PAD)
    t[:a.shape[0], :a.shape[1]] = a.to(dtype).to(DEV)
    return t


def _launch(layout, dims, H, hd, dtype, qkv, do):
    """vtx_attn_fwd + vtx_attn_bwd on guarded buffers.  Returns (out, lse, dqkv, dqkv_cls or None) as allocated."""
    from vtx import _lib as L_
    from vtx import ops
    S, L, B, T, P, rows, orows, rin, rout, grp = _geometry(layout, dims)
    D, W, n = H * hd, 3 * H * hd, S * H * L
    qd = _padded(qkv, dtype)
    if layout == 'space_nocls':
        qd[torch.arange(B, device=DEV) * (1 + P * T)] = float('nan')      # the cls rows of qkv are not read
    out = X.guarded((orows + 2, D), dtype, DEV, PAD)
    lse = X.sentinel_fill(torch.empty(n + PAD, device=DEV))
    d = L_.AttnDesc()
    d.dtype = L_.VTX_F32 if dtype == F32 else L_.VTX_BF16
    d.mode = {'contig': L_.ATTN_CONTIG, 'space': L_.ATTN_SPACE, 'time_cls': L_.ATTN_TIME_CLS, 'space_nocls': L_.ATTN_SPACE_NOCLS}[layout]
    d.S, d.L, d.H, d.hd, d.B, d.T, d.P = S, L, H, hd, B, T, P
    d.qkv, d.ld_qkv, d.out, d.ld_out, d.lse, d.probs, d.scale = qd.data_ptr(), W + PAD, out.data_ptr(), D + PAD, lse.data_ptr(), None, hd ** -0.5
    L_.call('vtx_attn_fwd', C.byref(d), ops.stream())
    dd = _padded(do, dtype)
    dqkv = X.guarded((rows + 2, W), dtype, DEV, PAD)
    dcls = X.guarded((S + 2, W), dtype, DEV, PAD) if grp else None
    delta = torch.empty(n, device=DEV)
    b = L_.AttnBwdDesc()
    b.f = d
    b.dout, b.ld_dout, b.dqkv, b.ld_dqkv, b.delta = dd.data_ptr(), D + PAD, dqkv.data_ptr(), W + PAD, delta.data_ptr()
    b.dqkv_cls = dcls.data_ptr() if grp else None
    L_.call('vtx_attn_bwd', C.byref(b), ops.stream())
    torch.cuda.synchronize()
    return out, lse, dqkv, dcls


def _untouched(tag, **regions):
    for name, t in regions.items():
        assert X.sentinel_touched(t) == 0, f'{tag}: {name} overwritten'


def _against_f64(layout, dims, H, hd, dtype, operands='random'):
    from vtx import _lib as L_
    from vtx import ops
    S, L, B, T, P, rows, orows, rin, rout, grp = _geometry(layout, dims)
    D, W, n = H * hd, 3 * H * hd, S * H * L
    qkv, do, r_out, r_lse, r_dqkv, r_cls = _reference(layout, dims, H, hd, dtype, operands)
    out, lse, dqkv, dcls = _launch(layout, dims, H, hd, dtype, qkv, do)
    tag = f'attn hd={hd} {layout} {dims} {IDS[dtype]}' + ('' if operands == 'random' else f' {operands}')
    _untouched(tag, ld_out_pad=out[:, D:], rows_after_out=out[orows:], lse_tail=lse[n:], ld_dqkv_pad=dqkv[:, W:], rows_after_dqkv=dqkv[rows:])
    check(f'{tag} out', out[:orows, :D].float().cpu(), r_out, TOL[dtype])
    check(f'{tag} lse', lse[:n].cpu().reshape(S, H, L), r_lse, LSE_BAR)
    cls_rows = torch.arange(B) * (1 + P * T)
    tok = torch.ones(rows, dtype=torch.bool)
    if layout != 'contig':
        tok[cls_rows] = False
    check(f'{tag} dqkv', dqkv[:rows, :W][tok.to(DEV)].float().cpu(), r_dqkv[tok], 2 * TOL[dtype])
    if layout == 'space_nocls':
        z = dqkv[cls_rows.to(DEV), :W]
        assert int((_bits(z.contiguous()) != 0).sum()) == 0, f'{tag}: the cls rows of dqkv are zeros'
    if grp:
        _untouched(tag, clip_cls_rows=dqkv[cls_rows.to(DEV)], ld_dcls_pad=dcls[:, W:], rows_after_dcls=dcls[S:])
        check(f'{tag} per-sequence cls rows', dcls[:S, :W].float().cpu(), r_cls, 2 * TOL[dtype])
        L_.call('vtx_cls_qkv_reduce', L_.VTX_F32 if dtype == F32 else L_.VTX_BF16, B, grp, W, dcls.data_ptr(), W + PAD, dqkv.data_ptr(),
                W + PAD, 1 + P * T, ops.stream())
        torch.cuda.synchronize()
        check(f'{tag} dqkv after cls_qkv_reduce', dqkv[:rows, :W].float().cpu(), r_dqkv, 2 * TOL[dtype])
        _untouched(tag, ld_dqkv_pad=dqkv[:, W:], rows_after_dqkv=dqkv[rows:])


@pytest.mark.parametrize('dtype', [F32, BF16], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('hd', HDS)
@pytest.mark.parametrize('L', [1, 8, 32, 33, 65, 129, 197, 257])
def test_contig_against_float64(L, hd, dtype):
    """Up to 32 tokens: the VALU kernels, packed; above: the VALU kernels (fp32) / attn_hd.hip (bf16)."""
    _against_f64('contig', (3, L), 2, hd, dtype)


@pytest.mark.parametrize('dtype', [F32, BF16], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('hd', HDS)
@pytest.mark.parametrize('layout,dims', [('space', (2, 3, 40)), ('space', (1, 2, 300)), ('time_cls', (2, 8, 5)), ('time_cls', (1, 40, 3)),
                                         ('space_nocls', (2, 3, 36)), ('space_nocls', (2, 3, 33))])
def test_layouts_against_float64(layout, dims, hd, dtype):
    _against_f64(layout, dims, 2, hd, dtype)


# ------------------------------------------------------------------------------------------------ 2. exact arithmetic
@functools.lru_cache(maxsize=None)
def _exact_contig(S, L, H, hd):
    return A.contig_case(S, L, H, hd=hd)


@functools.lru_cache(maxsize=None)
def _exact_space(B, T, P, H, hd):
    return A.space_case(B, T, P, H, hd=hd)


def _run_exact(c):
    """The runners of tests/test_gpu_exact_attention.py (the descriptor's scale is exact_attn.SCALE = 2^-3 at every head dim,
    as in the cross-attention tests): RNE equality on out, dqkv, the per-frame cls rows; the lse standard; the guards."""
    assert c.hd in HDS and c.L > 32
    qkv, out, lse = E.run_fwd(c, BF16)
    return (out, lse) + E.run_bwd(c, BF16, qkv, out, lse, True)


@pytest.mark.parametrize('hd', HDS)
@pytest.mark.parametrize('L', [33, 129, 257, 385])
def test_mfma_contig_exact(L, hd):
    _run_exact(_exact_contig(2, L, 2, hd))


@pytest.mark.parametrize('hd', HDS)
def test_mfma_space_exact(hd):
    _run_exact(_exact_space(2, 3, 130, 2, hd))


# ------------------------------------------------------------------------------------------------ 3. determinism
@pytest.mark.parametrize('hd', HDS)
def test_mfma_is_bit_reproducible(hd):
    for c in (_exact_contig(2, 385, 2, hd), _exact_space(2, 3, 130, 2, hd)):
        first, again = _run_exact(c), _run_exact(c)
        for a, b in zip(first, again):
            if a is not None:
                assert torch.equal(_bits(a), _bits(b)), 'second run differs'


# ------------------------------------------------------------------------------------------------ 4. mfma against valu
def _plain(S, L, H, hd, dtype, qkv, do):
    from vtx import ops
    from vtx._lib import ATTN_CONTIG
    D = H * hd
    o = torch.full((S, L, D), float('nan'), dtype=dtype, device=DEV)
    lse = torch.full((S * H * L,), float('nan'), device=DEV)
    ops.attn_fwd(qkv, o, lse, ATTN_CONTIG, S, L, H, hd, hd ** -0.5)
    dqkv = torch.full((S, L, 3 * D), float('nan'), dtype=dtype, device=DEV)
    ops.attn_bwd(qkv, o, lse, do, dqkv, ATTN_CONTIG, S, L, H, hd, hd ** -0.5)
    torch.cuda.synchronize()
    return o, lse, dqkv


@pytest.mark.parametrize('hd', HDS)
@pytest.mark.parametrize('L', [33, 197, 300])
def test_mfma_matches_valu(L, hd, attn_hd, vtx_opts):
    S, H = 2, 3
    qkv = dev(rnd(S, L, 3 * H * hd, seed=5) * 1.5, BF16)
    do = dev(rnd(S, L, H * hd, seed=6), BF16)
    new = _plain(S, L, H, hd, BF16, qkv, do)
    attn_hd('valu')
    old = _plain(S, L, H, hd, BF16, qkv, do)
    attn_hd('mfma')
    vtx_opts('attn_valu', '1')
    valu = _plain(S, L, H, hd, BF16, qkv, do)
    assert all(torch.isfinite(t.float()).all() for t in new)
    for a, b in zip(old, valu):
        assert torch.equal(_bits(a), _bits(b)), f'hd={hd} L={L}: attn_hd=valu differs from attn_valu=1'
    for what, a, b, bar in zip(('out', 'lse', 'dqkv'), new, old, (1e-2, 1e-4, 2e-2)):
        check(f'attn hd={hd} mfma vs valu {what} L={L}', a.float().cpu(), b.float().cpu(), bar)


@pytest.mark.parametrize('dtype,L', [(BF16, 8), (BF16, 197), (BF16, 300), (F32, 8), (F32, 40)])
def test_head_dim_64_ignores_attn_hd(dtype, L, attn_hd):
    S, H, hd = 2, 3, 64
    qkv = dev(rnd(S, L, 3 * H * hd, seed=5) * 1.5, dtype)
    do = dev(rnd(S, L, H * hd, seed=6), dtype)
    attn_hd('mfma')
    new = _plain(S, L, H, hd, dtype, qkv, do)
    attn_hd('valu')
    old = _plain(S, L, H, hd, dtype, qkv, do)
    for a, b in zip(new, old):
        assert torch.isfinite(a.float()).all() and torch.equal(_bits(a), _bits(b)), f'{IDS[dtype]} L={L}: attn_hd changes head_dim 64'


# ------------------------------------------------------------------------------------------------ 5. models
WIDTHS = [(64, 2), (192, 2), (256, 2)]                 # (embed_dims, num_heads): head_dim 32, 96, 128
PRECS = [('fp32', TOL_F32, TOL_F32), ('bf16', TOL_BF16, TOL_BF16_GRAD)]
CLIPS, FRAMES, IMG, PATCH, LAYERS = 2, 4, 48, 8, 2     # P = 36: spatial L = 37, temporal L = 4 (5 with the cls token), joint L = 145


def _step(m, x, d, run):
    """Forward + backward of loss = sum(y * w) in eval mode (DropPath off: no random numbers to keep in step with the oracle)."""
    m.eval()
    m.zero_grad()
    y = run(m, x.to(DEV))
    (y.float() * (synth_tensor('loss_w', (d,), 0) * 10.0).to(DEV)).sum().backward()
    torch.cuda.synchronize()
    return y.detach().float().cpu(), {k: p.grad.detach().float().cpu() for k, p in m.named_parameters() if p.grad is not None}


def _compare(tag, y, grads, yo, ps, prec, tol, gtol):
    check(f'{tag} {prec} out', y, yo.detach(), tol)
    assert grads and set(grads) <= set(ps)
    worst = 0.0
    for k, g in grads.items():
        ref = ps[k].grad
        e = relerr(g, ref) if prec == 'fp32' else l2err(g, ref)
        worst = max(worst, e)
        if e > gtol:
            report(f'FAIL {tag} {prec} grad {k}: {e:.3e} (tol {gtol:g})')
        assert e <= gtol, f'{tag} {prec}: grad {k} {"max-rel" if prec == "fp32" else "rel L2"} {e:.3e} > {gtol:g}'
    report(f'ok   {tag} {prec}: {len(grads)} parameter gradients, worst {worst:.3e} (tol {gtol:g})')


def _model_case(kind, d, heads, prec, tol, gtol, stream='bf16'):
    import vtx
    import video_transformer as V
    from model_common import _build
    vtx.set_precision(prec)
    vtx.set_stream(stream)
    cfg = dict(num_frames=FRAMES, img_size=IMG, patch_size=PATCH, embed_dims=d, num_heads=heads, num_transformer_layers=LAYERS)
    x = synth.synth_clip(CLIPS, FRAMES, 3, IMG, IMG, seed=2)
    w = synth_tensor('loss_w', (d,), 0) * 10.0
    if kind == 'vivit fact_encoder':
        m, sd = _build(V.ViViT, 4, attention_type='fact_encoder', **cfg)
        ps = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
        yo = O.vivit_forward(ps, x, FRAMES, heads=heads, layers=LAYERS)
    else:
        at = kind.split()[1]
        m, sd = _build(V.TimeSformer, 3, attention_type=at, **cfg)
        ps = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
        yo = O.timesformer_forward(ps, x, FRAMES, heads=heads, layers=LAYERS, attention_type=at)
    (yo * w).sum().backward()
    y, grads = _step(m, x, d, lambda mm, xx: mm(xx))
    _compare(f'{kind} hd={d // heads}' + (' exact stream' if stream != 'bf16' else ''), y, grads, yo, ps, prec, tol, gtol)


@pytest.mark.parametrize('prec,tol,gtol', PRECS, ids=['fp32', 'bf16'])
@pytest.mark.parametrize('d,heads', WIDTHS, ids=['hd32', 'hd96', 'hd128'])
@pytest.mark.parametrize('kind', ['tsf divided_space_time', 'tsf joint_space_time', 'vivit fact_encoder'])
def test_models_against_the_oracle(kind, d, heads, prec, tol, gtol):
    _model_case(kind, d, heads, prec, tol, gtol)


def test_exact_stream_against_the_oracle():
    _model_case('tsf divided_space_time', 192, 2, 'bf16', TOL_BF16, TOL_BF16_GRAD, stream='fp32')


def _space_then_time(x, sd, layers, T, heads):
    """The container with operator_order = ['space_attn', 'time_attn', 'ffn'] from the oracle's pieces: the spatial block leaves
    the cls token out (sequences = the P tokens of a frame; the cls row passes through), the temporal block takes it in (the
    cls row heads each of the P sequences of T tokens, its outputs are averaged over them, there is no temporal_fc)."""
    b, n1, d = x.shape
    P = (n1 - 1) // T
    for i in range(layers):
        pre = f'layers.{i}.attentions.0.'
        cls, tok = x[:, :1], x[:, 1:]
        fr = tok.reshape(b, P, T, d).permute(0, 2, 1, 3).reshape(b * T, P, d)
        a, _ = O.attention(O.layer_norm(fr, sd[pre + 'norm.weight'], sd[pre + 'norm.bias'], 1e-5), sd, pre + 'attn.', heads)
        x = torch.cat([cls, tok + a.reshape(b, T, P, d).permute(0, 2, 1, 3).reshape(b, P * T, d)], 1)
        pre = f'layers.{i}.attentions.1.'
        cls, tok = x[:, :1], x[:, 1:]
        seq = torch.cat([cls.unsqueeze(1).expand(b, P, 1, d), tok.reshape(b, P, T, d)], 2).reshape(b * P, 1 + T, d)
        a, _ = O.attention(O.layer_norm(seq, sd[pre + 'norm.weight'], sd[pre + 'norm.bias'], 1e-5), sd, pre + 'attn.', heads)
        a = a.reshape(b, P, 1 + T, d)
        x = x + torch.cat([a[:, :, 0].mean(1, keepdim=True), a[:, :, 1:].reshape(b, P * T, d)], 1)
        x = O.ffn_block(x, sd, f'layers.{i}.ffns.0.', 0.0, False)
    return x


@pytest.mark.parametrize('prec,tol,gtol', PRECS, ids=['fp32', 'bf16'])
@pytest.mark.parametrize('d,heads', WIDTHS, ids=['hd32', 'hd96', 'hd128'])
def test_space_then_time_container_against_the_oracle(d, heads, prec, tol, gtol):
    """The other operator order: VTX_ATTN_SPACE_NOCLS at L = 36, VTX_ATTN_TIME_CLS at L = 5."""
    import vtx
    import transformer as T_
    vtx.set_precision(prec)
    P = (IMG // PATCH) ** 2
    m = T_.TransformerContainer(num_transformer_layers=LAYERS, embed_dims=d, num_heads=heads, num_frames=FRAMES, hidden_channels=4 * d,
                                operator_order=['space_attn', 'time_attn', 'ffn'])
    sd = synth.synth_state_dict(synth.shapes_of(m), 7)
    m.load_state_dict(sd, strict=True)
    m.to(DEV)
    x = torch.from_numpy(np.random.RandomState(7).standard_normal((CLIPS, 1 + P * FRAMES, d)).astype(np.float32))
    ps = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    yo = _space_then_time(x, ps, LAYERS, FRAMES, heads)
    (yo * (synth_tensor('loss_w', (d,), 0) * 10.0)).sum().backward()
    ps = {k: v for k, v in ps.items() if v.grad is not None}            # (temporal_fc is not used in this order)
    y, grads = _step(m, x, d, lambda mm, xx: T_.stream_value(mm(xx)))
    grads = {k: g for k, g in grads.items() if k in ps}
    _compare(f'space-then-time container hd={d // heads}', y, grads, yo, ps, prec, tol, gtol)


@pytest.mark.parametrize('prec,tol', [('fp32', TOL_F32), ('bf16', TOL_BF16)])
def test_get_last_selfattention_against_the_oracle(prec, tol):
    """head_dim 96; the last attention of the divided model is the spatial one, [(b t), H, 37, 37]: the forward of its route
    and the VALU `probs` pass behind it."""
    import vtx
    import video_transformer as V
    from model_common import _build
    vtx.set_precision(prec)
    cfg = dict(num_frames=FRAMES, img_size=IMG, patch_size=PATCH, embed_dims=192, num_heads=2, num_transformer_layers=LAYERS)
    m, sd = _build(V.TimeSformer, 3, **cfg)
    x = synth.synth_clip(CLIPS, FRAMES, 3, IMG, IMG, seed=2)
    want = O.timesformer_forward(sd, x, FRAMES, heads=2, layers=LAYERS, return_attention=True)
    m.eval()
    with torch.no_grad():
        att = m.get_last_selfattention(x.to(DEV))
    assert tuple(att.shape) == tuple(want.shape) == (CLIPS * FRAMES, 2, 37, 37)
    check(f'tsf divided hd=96 {prec} last attention', att.float().cpu(), want, tol)
    assert abs(att.float().sum(-1).cpu() - 1).max().item() < 1e-3


# ------------------------------------------------------------------------------------------------ 6. head_dim 64 unchanged
@pytest.mark.parametrize('dtype,contig,space', [
    ('bfloat16', [(5, 8, 3), (2, 197, 3), (2, 300, 3)], [(2, 3, 8, 2), (1, 2, 196, 3)]),     # packed, 33..256, > 256; space VALU / MFMA
    ('float32', [(5, 8, 3), (2, 197, 3)], [(2, 3, 36, 2)])])                                  # VALU, exact-fp32 MFMA
def test_head_dim_64_is_the_parent_bit_for_bit(dtype, contig, space, tmp_path):
    spec = dict(dtype=dtype, options={}, contig=[list(c) for c in contig], space=[list(c) for c in space])
    assert_parent_bit_for_bit(spec, tmp_path, f'head_dim 64 {dtype}')
