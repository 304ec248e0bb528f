"""Dropout on the HIP path (csrc/dropout.hip, include/vtx_dropout.h vtx_dropout_rows): proj_drop, the FFN's dropout_p and the embedding
dropout_p of TimeSformer / ViViT.  attn_drop stays refused.

  1. the kernel against the NumPy restatement of the mask contract (tests/dropout_ref.py), bit for bit, fp32 and bf16: row maps,
     residual, row scale, time-embedding table, in place and out of place, both ends of p, two sites, an element offset that
     reaches the high counter word, and a launch just above the grid cap (the cap comes from vtx.ops);
  2. placement through every Function, exact: under vtx.set_stream('fp32') with DropPath off a sub-block returns its contribution
     alone, which is zero exactly on the dropped set of its last site and non-zero elsewhere (random normal inputs: a bf16 zero
     would need |t| < 2^-133).  The test re-derives the seed by re-seeding the CPU generator and repeating the documented draws;
  3. parity with the masks known: the sub-blocks, TimeSformer and ViViT against a float64 torch composition written here from the
     oracle's pieces, the helper's masks and the DropPath vector the module drew -- fp32 within TOL_F32, bf16 within TOL_BF16 /
     TOL_BF16_GRAD with ELEMENT_SLACK (the project's own bars);
  4. nothing moves at p == 0: training with p = 0 and eval with p = 0.3 equal the module built without dropout arguments, bit
     for bit, outputs, gradients and the CPU generator's state;
  5. recompute against stored activations, bit for bit; what is still refused.
"""
import numpy as np
import pytest
import torch

import dropout_ref as R
import helpers
from helpers import ELEMENT_SLACK, TOL_BF16, TOL_BF16_GRAD, TOL_F32
from model_common import SMALL, _build
from oracle import synth, vt_oracle as O

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
BF16, F32 = torch.bfloat16, torch.float32
SEED = 0x9abcdef012345678
D_, HEADS, HIDDEN, FRAMES, PATCHES, CLIPS = 128, 2, 512, 2, 16, 2
KINDS = ['ffn', 'self', 'time', 'time_cls', 'space', 'space_nocls']


@pytest.fixture(autouse=True)
def _reset_modes():
    import vtx
    yield
    vtx.set_precision('auto')
    vtx.set_stream('bf16')
    vtx.set_recompute(False)


def _vals(shape, seed, bf16):
    x = np.random.RandomState(seed).randn(*shape).astype(np.float32)
    return R.bf16_round(x) if bf16 else x


def _dev(a, bf16):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t.to(BF16) if bf16 else t


def _same(t, ref):
    got = t.float().cpu()
    want = torch.from_numpy(np.ascontiguousarray(ref))
    assert torch.equal(got, want), f'{(got != want).sum().item()} of {want.numel()} elements differ'


# ---------------------------------------------------------------------------------------------------------------- 1. the kernel
@pytest.mark.parametrize('bf16', [False, True], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('p', [0.1, 0.5])
def test_kernel_identity_maps(bf16, p):
    from vtx import ops
    x = _vals((7, 40), 1, bf16)
    want = R.apply(x, SEED, 0, p, bf16=bf16)
    assert (want == 0).any() and (want != 0).any()
    xd = _dev(x, bf16)
    y = torch.full_like(xd, 7.0)
    ops.dropout_rows(xd, y, 7, 40, p, SEED, 0)
    _same(y, want)
    _same(xd, x)                                         # out of place: the source is not modified
    ops.dropout_rows(xd, xd, 7, 40, p, SEED, 0)          # in place
    _same(xd, want)


@pytest.mark.parametrize('bf16', [False, True], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('p', [0.1, 0.5])
def test_kernel_token_map_residual_and_row_scale(bf16, p):
    """2 clips x (1 + 6) tokens x 40 through tokmap(6): the logical row m = b 6 + n indexes the mask, the residual and the output
    take the row map, the per-clip scale s[m / 6]; the cls rows are not touched."""
    from vtx import ops
    x, post = _vals((2, 7, 40), 2, bf16), _vals((2, 7, 40), 3, bf16)
    s = np.asarray([0.75, 1.25], np.float32)
    tok = R.apply(x[:, 1:].reshape(12, 40), SEED, 1, p, s=np.repeat(s, 6), post=post[:, 1:].reshape(12, 40), bf16=bf16)
    tm = ops.tokmap(6)
    for in_place in (False, True):
        xd, pd = _dev(x, bf16), _dev(post, bf16)
        y = xd if in_place else torch.full_like(xd, 7.0)
        want = x.copy() if in_place else np.full_like(x, 7.0)
        want[:, 1:] = tok.reshape(2, 6, 40)
        ops.dropout_rows(xd, y, 12, 40, p, SEED, 1, xmap=tm, ymap=tm, post=pd, pmap=tm, s=_dev(s, False), rs=(6, 1, 1, 0))
        _same(y, want)


@pytest.mark.parametrize('bf16', [False, True], ids=['fp32', 'bf16'])
def test_kernel_pre_table_of_period_3(bf16):
    from vtx import ops
    x, pre = _vals((7, 40), 4, bf16), _vals((3, 40), 5, False)
    want = R.apply(x, SEED, 1, 0.5, pre=pre[np.arange(7) % 3], bf16=bf16)
    xd = _dev(x, bf16)
    y = torch.empty_like(xd)
    ops.dropout_rows(xd, y, 7, 40, 0.5, SEED, 1, pre=_dev(pre, False), pre_period=3)
    _same(y, want)


@pytest.mark.parametrize('bf16', [False, True], ids=['fp32', 'bf16'])
def test_kernel_ends_of_p_sites_and_high_counter_word(bf16):
    from vtx import ops
    x, post = _vals((7, 40), 6, bf16), _vals((7, 40), 7, bf16)
    xd, pd = _dev(x, bf16), _dev(post, bf16)
    y = torch.full_like(xd, float('nan'))
    ops.dropout_rows(xd, y, 7, 40, 1.0, SEED, 0)         # p = 1: thr = 2^32, scale = 0: all zeros, no NaN
    _same(y, np.zeros_like(x))
    ops.dropout_rows(xd, y, 7, 40, 1.0, SEED, 0, post=pd)
    _same(y, post)                                       # ... or the residual alone
    assert ops.dropout_params(0.0) == (0, 1.0)
    ops.dropout_rows(xd, y, 7, 40, 0.0, SEED, 0)         # p = 0: thr = 0: the input
    _same(y, x)
    y0, y1, yh = torch.empty_like(xd), torch.empty_like(xd), torch.empty_like(xd)
    ops.dropout_rows(xd, y0, 7, 40, 0.5, SEED, 0)
    ops.dropout_rows(xd, y1, 7, 40, 0.5, SEED, 1)
    assert not torch.equal(y0, y1)                       # the sites of one seed differ
    _same(y1, R.apply(x, SEED, 1, 0.5, bf16=bf16))
    ops.dropout_rows(xd, yh, 7, 40, 0.5, SEED, 0, e0=2 ** 34)
    _same(yh, R.apply(x, SEED, 0, 0.5, e0=2 ** 34, bf16=bf16))
    assert not torch.equal(yh, y0)


def test_kernel_second_trip_of_the_capped_grid():
    """One launch just above the grid cap (vtx.ops.DROPOUT_TRIP elements per trip): the tail runs in the second trip."""
    from vtx import ops
    D = 40
    rows = ops.DROPOUT_TRIP // D + 5
    assert (rows - 1) * D >= ops.DROPOUT_TRIP > (rows - 6) * D
    x = np.ones((rows, D), np.float32)
    want = R.apply(x, SEED, 0, 0.5, bf16=True)
    xd = _dev(x, True)
    ops.dropout_rows(xd, xd, rows, D, 0.5, SEED, 0)
    _same(xd, want)


@pytest.mark.parametrize('dtype', [F32, BF16], ids=['fp32', 'bf16'])
def test_dropout_fn_backward_is_the_forward_on_dy(dtype):
    from vtx import functions as F_
    bf16 = dtype == BF16
    x = _dev(_vals((3, 5, 40), 8, bf16), bf16).requires_grad_(True)
    dy = _dev(_vals((3, 5, 40), 9, bf16), bf16)
    y = F_.DropoutFn.apply(x, 0.25, SEED, 1)
    y.backward(dy)
    _same(y.detach().reshape(15, 40), R.apply(x.detach().float().cpu().numpy().reshape(15, 40), SEED, 1, 0.25, bf16=bf16))
    assert torch.equal(x.grad, F_.DropoutFn.apply(dy, 0.25, SEED, 1))


# ------------------------------------------------------------------------------------------------------------ the sub-blocks
def _randomise(m, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, prm in m.named_parameters():
            v = torch.randn(prm.shape, generator=g) * (0.1 if prm.ndim > 1 else 0.05)
            if name.endswith('norm.weight'):
                v = v + 1.0
            prm.copy_(v)
    return m


def _block(kind, p=None, dp=0.0, seed=11):
    """The sub-block of `kind`; p None: built without any dropout argument."""
    import transformer as T
    ld = dict(type=T.DropPath, dropout_p=dp)
    if kind == 'ffn':
        kw = {} if p is None else dict(dropout_p=p)
        m = T.FFNWithPreNorm(embed_dims=D_, hidden_channels=HIDDEN, layer_drop=ld, **kw)
    else:
        kw = {} if p is None else dict(proj_drop=p)
        if kind == 'self':
            m = T.MultiheadAttentionWithPreNorm(embed_dims=D_, num_heads=HEADS, layer_drop=ld, **kw)
        else:
            cls = T.DividedTemporalAttentionWithPreNorm if kind.startswith('time') else T.DividedSpatialAttentionWithPreNorm
            m = cls(embed_dims=D_, num_heads=HEADS, num_frames=FRAMES, use_cls_token=kind in ('time_cls', 'space'), layer_drop=ld, **kw)
    return _randomise(m, seed).to(DEV)


def _block_input(seed=12):
    x = torch.randn(CLIPS, 1 + PATCHES * FRAMES, D_, generator=torch.Generator().manual_seed(seed))
    return x.to(BF16).float()                            # bf16 numbers: both precisions read the same input


def _droppath_rows(kind):
    return {'ffn': CLIPS, 'self': CLIPS, 'time': CLIPS * PATCHES, 'time_cls': CLIPS * PATCHES, 'space': CLIPS * FRAMES,
            'space_nocls': CLIPS * FRAMES}[kind]


def _draws(kind, gen_seed, dp, with_seed=True):
    """Repeat a sub-block forward's draws from the CPU generator: the DropPath vector (transformer.DropPath.scale_vector's
    arithmetic), then the dropout seed.  -> (scale vector float32 [rows] or None, seed)."""
    torch.manual_seed(gen_seed)
    s = None
    if dp:
        u = torch.rand((_droppath_rows(kind), 1, 1))
        s = np.floor(np.float32(1 - dp) + u.numpy().reshape(-1)) / np.float32(1 - dp)
    seed = int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64)) if with_seed else None
    return s, seed


def _mk(seed, site, e0, rows, D, p):
    """The helper's mask times the keep scale, float64."""
    return torch.from_numpy(R.keep_mask(seed, site, e0, rows, D, p).astype(np.float64)) * float(R.keep_scale(p))


def _ref_block(kind, x, sd, p, seed, s):
    """float64 composition of the sub-block of `kind` with the masks known (reference transformer.py:176,234-282,336-382,
    428-456,498-523): LayerNorm, Linear, GELU, softmax attention from the oracle's pieces."""
    B, N1, D = x.shape
    T = FRAMES
    ln = lambda t: O.layer_norm(t, sd['norm.weight'], sd['norm.bias'], 1e-5)       # noqa: E731
    one = torch.ones(_droppath_rows(kind), dtype=torch.float64)
    s = one if s is None else torch.from_numpy(s.astype(np.float64))
    if kind == 'ffn':
        g = O.gelu_erf(O.linear(ln(x), sd['layers.0.0.weight'], sd['layers.0.0.bias']))
        g = g * _mk(seed, 0, 0, B * N1, g.shape[-1], p).reshape(B, N1, -1)
        z = O.linear(g, sd['layers.1.weight'], sd['layers.1.bias']) * _mk(seed, 1, 0, B * N1, D, p).reshape(B, N1, D)
        return x + z * s.reshape(B, 1, 1)
    if kind == 'self':
        a = O.attention(ln(x), sd, 'attn.', HEADS)[0] * _mk(seed, 0, 0, B * N1, D, p).reshape(B, N1, D)
        return x + a * s.reshape(B, 1, 1)
    N = N1 - 1
    P = N // T
    cls, tok = x[:, :1], x[:, 1:]
    if kind == 'time':                                   # sequences (b, p) of T tokens; the mask sits in front of temporal_fc
        a = O.attention(ln(tok.reshape(B * P, T, D)), sd, 'attn.', HEADS)[0]
        a = a * _mk(seed, 0, 0, B * N, D, p).reshape(B * P, T, D) * s.reshape(B * P, 1, 1)
        a = O.linear(a, sd['temporal_fc.weight'], sd['temporal_fc.bias'])
        return torch.cat([cls, tok + a.reshape(B, N, D)], dim=1)
    if kind == 'time_cls':                               # sequences (b, p) of the cls row + T tokens; cls mean over p
        seq = torch.cat([cls.expand(B, P, D).reshape(B * P, 1, D), tok.reshape(B * P, T, D)], dim=1)
        a = O.attention(ln(seq), sd, 'attn.', HEADS)[0]
        m = _mk(seed, 0, 0, B * N + B * P, D, p)
        at = a[:, 1:] * m[:B * N].reshape(B * P, T, D) * s.reshape(B * P, 1, 1)
        ac = a[:, 0] * m[B * N:] * s.reshape(B * P, 1)
        return x + torch.cat([ac.reshape(B, P, D).mean(1, keepdim=True), at.reshape(B, N, D)], dim=1)
    frames = tok.reshape(B, P, T, D).permute(0, 2, 1, 3).reshape(B * T, P, D)
    back = lambda t: t.reshape(B, T, P, D).permute(0, 2, 1, 3).reshape(B, N, D)    # noqa: E731
    if kind == 'space':                                  # sequences (b, t) of the cls row + P tokens; cls mean over t
        seq = torch.cat([cls.expand(B, T, D).reshape(B * T, 1, D), frames], dim=1)
        a = O.attention(ln(seq), sd, 'attn.', HEADS)[0]
        m = _mk(seed, 0, 0, B * N + B * T, D, p)
        at = back(a[:, 1:] * s.reshape(B * T, 1, 1)) * m[:B * N].reshape(B, N, D)
        ac = a[:, 0] * m[B * N:] * s.reshape(B * T, 1)
        return x + torch.cat([ac.reshape(B, T, D).mean(1, keepdim=True), at], dim=1)
    assert kind == 'space_nocls'                         # sequences (b, t) of P tokens; the cls rows pass through
    a = O.attention(ln(frames), sd, 'attn.', HEADS)[0]
    at = back(a * s.reshape(B * T, 1, 1)) * _mk(seed, 0, 0, B * N, D, p).reshape(B, N, D)
    return torch.cat([cls, tok + at], dim=1)


def _run_block(m, x, gen_seed, w):
    m.zero_grad()
    xd = x.to(DEV).requires_grad_(True)
    torch.manual_seed(gen_seed)
    y = m(xd)
    state = torch.get_rng_state()
    (y.float() * w.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    grads = {k: prm.grad.clone() for k, prm in m.named_parameters() if prm.grad is not None}
    return y.detach(), xd.grad.clone(), grads, state


def _loss_w(shape, seed=13):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def _check_against(name, prec, y, dx, grads, y64, dx64, g64):
    """fp32: every element within TOL_F32 of max|ref|.  bf16: outputs within TOL_BF16, gradients within TOL_BF16_GRAD in relative
    L2 and every element within ELEMENT_SLACK * TOL_BF16_GRAD of max|ref|."""
    if prec == 'fp32':
        helpers.check(f'dropout {name} fp32 out', y, y64, TOL_F32)
        for k, ref in [('dx', dx64)] + sorted(g64.items()):
            helpers.check(f'dropout {name} fp32 grad {k}', dx if k == 'dx' else grads[k], ref, TOL_F32)
        return
    helpers.check(f'dropout {name} bf16 out', y, y64, TOL_BF16)
    for k, ref in [('dx', dx64)] + sorted(g64.items()):
        got = dx if k == 'dx' else grads[k]
        l2, mx = helpers.l2err(got, ref), helpers.relerr(got, ref)
        print(f'dropout {name} bf16 grad {k}: l2 {l2:.3e} max {mx:.3e}')
        assert l2 <= TOL_BF16_GRAD and mx <= ELEMENT_SLACK * TOL_BF16_GRAD, (name, k, l2, mx)


# ------------------------------------------------------------------------------------------------------------ 2. placement
@pytest.mark.parametrize('kind', KINDS)
def test_placement_of_the_last_site_is_exact(kind):
    import vtx
    import transformer as T
    vtx.set_precision('bf16')
    vtx.set_stream('fp32')
    p = 0.5
    m = _block(kind, p=p).train()
    if kind == 'time':                                   # the mask sits in front of temporal_fc: the identity shows it (exact in bf16)
        with torch.no_grad():
            m.temporal_fc.weight.copy_(torch.eye(D_))
            m.temporal_fc.bias.zero_()
    x = _block_input().to(DEV).to(BF16)
    torch.manual_seed(21)
    out = m(x)
    assert isinstance(out, T.Stream)
    d = out.d.detach().float().cpu().numpy()
    _, seed = _draws(kind, 21, 0.0)
    B, N1, D = d.shape
    N = N1 - 1
    if kind == 'ffn':
        got, keep = d.reshape(B * N1, D), R.keep_mask(seed, 1, 0, B * N1, D, p)
    elif kind == 'self':
        got, keep = d.reshape(B * N1, D), R.keep_mask(seed, 0, 0, B * N1, D, p)
    else:                                                # the token rows: rows 0 .. B N of o's order
        got, keep = d[:, 1:].reshape(B * N, D), R.keep_mask(seed, 0, 0, B * N, D, p)
    assert 0.4 < keep.mean() < 0.6
    assert not got[~keep].any(), f'{np.count_nonzero(got[~keep])} dropped elements are not zero'
    assert got[keep].all(), f'{np.count_nonzero(got[keep] == 0)} kept elements are zero'


# ------------------------------------------------------------------------------------------------------------ 3. parity
@pytest.mark.parametrize('prec', ['fp32', 'bf16'])
@pytest.mark.parametrize('kind,dp', [(k, 0.0) for k in KINDS] + [(k, 0.25) for k in KINDS])
def test_sub_block_parity_with_known_masks(kind, dp, prec):
    import vtx
    vtx.set_precision(prec)
    p = 0.25
    m = _block(kind, p=p, dp=dp).train()
    x, w = _block_input(), _loss_w((CLIPS, 1 + PATCHES * FRAMES, D_))
    y, dx, grads, _ = _run_block(m, x, 31, w)
    s, seed = _draws(kind, 31, dp)
    if dp:
        print(f'{kind}: DropPath drops {int((s == 0).sum())} of {s.size} groups')
    sd ={k: v.detach().double().cpu().requires_grad_(True) for k, v in m.state_dict().items()}
    x64 = x.double().requires_grad_(True)
    y64 = _ref_block(kind, x64, sd, p, seed, s)
    (y64 * w.double()).sum().backward()
    g64 = {k: v.grad for k, v in sd.items() if v.grad is not None}
    assert sorted(g64) == sorted(grads)
    _check_against(f'{kind} dp={dp}', prec, y, dx, grads, y64.detach(), x64.grad, g64)


def _droppath_off(m):
    import transformer as T
    for mod in m.modules():
        if isinstance(mod, T.DropPath):
            mod.dropout_p = 0.0
    return m


MODELS = {'tsf_divided': ('TimeSformer', dict(num_frames=2, attention_type='divided_space_time'), 2),
          'tsf_space_only': ('TimeSformer', dict(num_frames=2, attention_type='space_only'), 2),
          'vivit_fact': ('ViViT', dict(num_frames=4, attention_type='fact_encoder'), 4),
          'vivit_joint': ('ViViT', dict(num_frames=4, attention_type='joint_space_time'), 4)}


def _ref_model(name, sd, x, p, seed, dpr):
    """float64 composition of the model with the embedding masks known: the stream has one cls row per clip, masked once per site
    (drop_after_pos over every row of the stream, drop_after_time over the token rows and then the cls rows)."""
    b = x.shape[0]
    tok = O.patch_embed(x, sd)                           # [(b t), P, D]
    bt, P, D = tok.shape
    T = bt // b
    x0 = torch.cat([sd['cls_token'].expand(bt, 1, D), tok], dim=1) + sd['pos_embed']
    if name in ('tsf_space_only', 'vivit_fact'):         # the stream is [(b t), 1 + P, D]
        h = x0 * _mk(seed, 0, 0, bt * (1 + P), D, p).reshape(bt, 1 + P, D)
        if name == 'tsf_space_only':
            h = O.container(h, sd, 'transformer_layers.', 2, ['self_attn', 'ffn'], T, HEADS, True, drop_path_rate=dpr)
            h = h.reshape(b, -1, h.shape[1], h.shape[2]).mean(dim=1)
        else:
            h = O.container(h, sd, 'transformer_layers.0.', 2, ['self_attn', 'ffn'], T, HEADS, True, drop_path_rate=dpr)
            h = torch.cat([h[:b, 0:1], h[:, 1:].reshape(b, T, P, D).mean(dim=2)], dim=1) + sd['time_embed']
            h = h * _mk(seed, 1, 0, b * (1 + T), D, p).reshape(b, 1 + T, D)
            h = O.container(h, sd, 'transformer_layers.1.', 4, ['self_attn', 'ffn'], T, HEADS, True, drop_path_rate=dpr)
    else:                                                # the stream is [b, 1 + P T, D], token 1 + p T + t
        N = P * T
        body = x0[:, 1:].reshape(b, T, P, D).permute(0, 2, 1, 3).reshape(b, N, D)
        h = torch.cat([x0[:b, 0:1], body], dim=1) * _mk(seed, 0, 0, b * (1 + N), D, p).reshape(b, 1 + N, D)
        t_emb = sd['time_embed'].reshape(1, 1, T, D).expand(b, P, T, D).reshape(b, N, D)
        toks = (h[:, 1:] + t_emb) * _mk(seed, 1, 0, b * N, D, p).reshape(b, N, D)
        cls = h[:, :1] * _mk(seed, 1, b * N * D, b, D, p).reshape(b, 1, D)
        ops_ = ['time_attn', 'space_attn', 'ffn'] if name == 'tsf_divided' else ['self_attn', 'ffn']
        h = O.container(torch.cat([cls, toks], dim=1), sd, 'transformer_layers.', 2, ops_, T, HEADS, True, drop_path_rate=dpr)
    return O.layer_norm(h, sd['norm.weight'], sd['norm.bias'], 1e-6)[:, 0]


def _model(name, dropout_p=None, seed=3):
    import video_transformer as V
    cls, kw, frames = MODELS[name]
    kw = dict(kw, **SMALL)
    if dropout_p is not None:
        kw['dropout_p'] = dropout_p
    m, sd = _build(getattr(V, cls), seed, **kw)
    return m, sd, synth.synth_clip(2, frames, 3, 64, 64, seed=2)


@pytest.mark.parametrize('prec', ['fp32', 'bf16'])
@pytest.mark.parametrize('name,dpr', [(n, 0.0) for n in MODELS] + [(n, 0.1) for n in MODELS])
def test_model_parity_with_known_masks(name, dpr, prec):
    import vtx
    vtx.set_precision(prec)
    p = 0.25
    m, sd, x = _model(name, p)
    if not dpr:
        _droppath_off(m)
    m.train()
    m.zero_grad()
    w = _loss_w((2, D_))
    torch.manual_seed(41)
    y = m(x.to(DEV))
    (y * w.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    grads = {k: prm.grad for k, prm in m.named_parameters() if prm.grad is not None}
    sd64 = {k: v.detach().double().requires_grad_(True) for k, v in sd.items()}
    torch.manual_seed(41)
    seed = int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64))      # prepare_tokens draws first, the blocks after it
    y64 = _ref_model(name, sd64, x.double(), p, seed, dpr)
    (y64 * w.double()).sum().backward()
    g64 = {k: v.grad for k, v in sd64.items() if v.grad is not None}
    assert sorted(g64) == sorted(grads)
    first = sorted(g64)[0]
    _check_against(f'{name} dpr={dpr}', prec, y.detach(), grads[first], grads, y64.detach(), g64[first], g64)


# ------------------------------------------------------------------------------------------------------------ 4. p == 0
@pytest.mark.parametrize('prec', ['fp32', 'bf16'])
@pytest.mark.parametrize('kind', KINDS)
def test_nothing_moves_at_p_zero(kind, prec):
    import vtx
    vtx.set_precision(prec)
    x, w = _block_input(), _loss_w((CLIPS, 1 + PATCHES * FRAMES, D_))
    for p, train in ((0.0, True), (0.3, False)):
        plain, drop = _block(kind, None, dp=0.25).train(train), _block(kind, p, dp=0.25).train(train)
        a, b = _run_block(plain, x, 51, w), _run_block(drop, x, 51, w)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), (kind, p)
        assert sorted(a[2]) == sorted(b[2]) and all(torch.equal(a[2][k], b[2][k]) for k in a[2]), (kind, p)
        assert torch.equal(a[3], b[3]), 'the CPU generator moved'


@pytest.mark.parametrize('name', ['tsf_divided', 'vivit_fact'])
def test_nothing_moves_at_p_zero_models(name):
    import vtx
    vtx.set_precision('bf16')
    for p, train in ((0.0, True), (0.3, False)):
        outs = []
        for dropout_p in (None, p):
            m, _, x = _model(name, dropout_p)
            m.train(train)
            torch.manual_seed(61)
            y = m(x.to(DEV))
            state = torch.get_rng_state()
            y.sum().backward()
            outs.append((y.detach(), {k: prm.grad for k, prm in m.named_parameters()}, state))
        (ya, ga, sa), (yb, gb, sb) = outs
        assert torch.equal(ya, yb) and torch.equal(sa, sb)
        assert all(torch.equal(ga[k], gb[k]) for k in ga)


# ------------------------------------------------------------------------------------------------------------ 5. recompute, refusals
def test_recompute_redraws_the_same_masks():
    """torch.utils.checkpoint restores the CPU generator around the re-run: the sub-blocks' seeds come out the same.  The blocks
    of a model take no dropout argument from its constructor (as in the reference), so the test switches theirs on by hand."""
    import vtx
    import transformer as T
    vtx.set_precision('bf16')
    m, _, x = _model('tsf_divided', 0.25)
    for mod in m.modules():
        if isinstance(mod, T.FFNWithPreNorm):
            mod.dropout_p = 0.25
        elif hasattr(mod, 'proj_drop') and hasattr(mod, 'layer_drop'):
            mod.proj_drop.p = 0.25
    m.train()
    res = []
    for on in (False, True):
        vtx.set_recompute(on)
        m.zero_grad()
        torch.manual_seed(71)
        y = m(x.to(DEV))
        y.sum().backward()
        res.append((y.detach().clone(), {k: prm.grad.clone() for k, prm in m.named_parameters()}))
    assert torch.equal(res[0][0], res[1][0])
    assert all(torch.equal(res[0][1][k], res[1][1][k]) for k in res[0][1])
    vtx.set_recompute(False)
    m.zero_grad()
    torch.manual_seed(72)                                # another seed: other masks (the test above is not vacuous)
    assert not torch.equal(m(x.to(DEV)).detach(), res[0][0])


def test_attn_drop_is_still_refused():
    import transformer as T
    ld = lambda: dict(type=T.DropPath, dropout_p=0.0)    # noqa: E731
    x = _block_input().to(DEV)
    mods = [T.MultiheadAttentionWithPreNorm(embed_dims=D_, num_heads=HEADS, attn_drop=0.1, layer_drop=ld()),
            T.DividedTemporalAttentionWithPreNorm(D_, HEADS, FRAMES, False, attn_drop=0.1, layer_drop=ld()),
            T.DividedTemporalAttentionWithPreNorm(D_, HEADS, FRAMES, True, attn_drop=0.1, layer_drop=ld()),
            T.DividedSpatialAttentionWithPreNorm(D_, HEADS, FRAMES, True, attn_drop=0.1, layer_drop=ld()),
            T.DividedSpatialAttentionWithPreNorm(D_, HEADS, FRAMES, False, attn_drop=0.1, layer_drop=ld()),
            T.Attention(D_, HEADS, qkv_bias=True, attn_drop=0.1)]
    for m in mods:
        m.to(DEV).train()
        with pytest.raises(NotImplementedError, match='attn_drop'):
            m(x)
        m.eval()
        m(x)                                             # eval: an identity, as before


def test_attention_module_proj_drop():
    """Attention.forward: LinearFn then DropoutFn, site 0 over the [B N, D] rows."""
    import vtx
    import transformer as T
    vtx.set_precision('fp32')
    m = _randomise(T.Attention(D_, HEADS, qkv_bias=True, proj_drop=0.5), 5).to(DEV).train()
    x = _block_input().to(DEV)
    torch.manual_seed(81)
    y, probs = m(x)
    seed = _draws('self', 81, 0.0)[1]
    m.eval()
    y0, probs0 = m(x)
    assert torch.equal(probs, probs0)
    keep = torch.from_numpy(R.keep_mask(seed, 0, 0, x.shape[0] * x.shape[1], D_, 0.5)).reshape(y.shape).to(DEV)
    assert torch.equal(y, torch.where(keep, y0 * 2, torch.zeros_like(y0)))


def test_embedding_dropout_under_the_exact_stream_is_refused():
    import vtx
    vtx.set_precision('bf16')
    vtx.set_stream('fp32')
    m, _, x = _model('tsf_divided', 0.25)
    m.train()
    with pytest.raises(NotImplementedError, match='embedding dropout'):
        m(x.to(DEV))
    m.eval()
    m(x.to(DEV))
