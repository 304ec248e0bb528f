"""vtx.set_stream('fp32'): the exact residual stream of the bf16 path (round 6).

The default bf16 path stores the residual stream as bf16: every sub-block's x + f(x) is rounded, and the error of the running sum
grows with sqrt(depth) -- measured on the REFERENCE's own arithmetic (tests/golden/make_golden_r6.py, tools/precision_study_l96.py):
its torch.autocast(bfloat16) run deviates by 5.0e-3 on TimeSformer-L / 96 frames at 24 layers, 1.43e-2 once its stream is rounded to
bf16 after every sub-block.  Under the exact stream a sub-block hands on its contribution and the running sum lives in float32
(vtx_layernorm_acc_fwd).  These tests hold that mode against the SAME goldens as the default mode with the FIXED bars (no
calibration, no widening), and against the reference's own autocast deviation where the golden carries it.
"""
import pytest
import torch

from helpers import TOL_BF16, TOL_BF16_GRAD, cal_entry, check, compare_grads, gold, relerr, report
from model_common import DEV, SMALL, _build, _reset_precision, _train_step  # noqa: F401
from oracle import synth, vt_oracle as O
from oracle.synth import synth_tensor

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _exact_stream():
    import vtx
    vtx.set_precision('bf16')
    vtx.set_stream('fp32')
    yield
    vtx.set_stream('bf16')


def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize('D', [128, 200, 768, 1024])
@pytest.mark.parametrize('with_xs', [True, False])
def test_layernorm_acc_fwd_vs_float64(D, with_xs):
    """vtx_layernorm_acc_fwd: xo = xs + d (float32; xs absent: d) on the mapped rows, y = LayerNorm(xo) in bf16, statistics of the
    float32 row; token map on the stream side (the cls row of every clip is skipped), accumulate-only form on the cls rows."""
    from vtx import ops
    B, N = 3, 37
    xs = (rnd(B, 1 + N, D, seed=1) * 3 + 0.5).to(DEV)
    d = (rnd(B, 1 + N, D, seed=2) * 0.3).bfloat16().to(DEV)
    gamma, beta = (1 + 0.1 * rnd(D, seed=3)).to(DEV), (0.1 * rnd(D, seed=4)).to(DEV)
    xo = torch.full((B, 1 + N, D), float('nan'), device=DEV)
    y = torch.empty(B * N, D, dtype=torch.bfloat16, device=DEV)
    mean, rstd = torch.empty(B * N, device=DEV), torch.empty(B * N, device=DEV)
    tm = ops.tokmap(N)
    ops.layernorm_acc_fwd(xs if with_xs else None, d, B * N, D, D, tm, xo, D, tm, gamma, beta, 1e-5, y, D, ops.IDENT, mean, rstd)
    ops.layernorm_acc_fwd(xs if with_xs else None, d, B, D, D, ops.clsmap(N), xo, D, ops.clsmap(N))
    torch.cuda.synchronize()
    ref = (xs.double() if with_xs else 0) + d.double()
    assert torch.equal(xo.cpu(), ref.float().cpu()), 'the float32 stream is the exactly rounded sum'
    ln = torch.nn.functional.layer_norm(xo.double()[:, 1:], (D,), gamma.double(), beta.double(), 1e-5).reshape(B * N, D)
    check(f'ln_acc_fwd y D={D} xs={with_xs}', y.float().cpu(), ln.cpu(), 1e-2)
    check(f'ln_acc_fwd mean D={D} xs={with_xs}', mean.cpu(), xo[:, 1:].double().mean(-1).reshape(-1).cpu(), 1e-5)


def test_layernorm_bwd_with_a_float32_stream():
    """vtx_layernorm_bwd, dtype VTX_BF16_X32: gradients bf16, the saved x float32 -- against float64."""
    from vtx import ops
    B, N, D = 3, 37, 768
    x = (rnd(B, 1 + N, D, seed=1) * 2 + 0.5)
    gamma = 1 + 0.1 * rnd(D, seed=2)
    dy = rnd(B * N, D, seed=4).bfloat16()
    dres = rnd(B, 1 + N, D, seed=5).bfloat16()
    xq = x.double().requires_grad_(True)
    gq, bq = gamma.double().requires_grad_(True), torch.zeros(D, dtype=torch.float64, requires_grad=True)
    ref = torch.nn.functional.layer_norm(xq[:, 1:], (D,), gq, bq, 1e-5).reshape(B * N, D)
    ref.backward(dy.double())
    dx_ref = xq.grad + dres.double()
    dx_ref[:, 0] = 0
    tm = ops.tokmap(N)
    xd = x.to(DEV)
    mean = xd[:, 1:].mean(-1).reshape(-1).contiguous()
    rstd = (xd[:, 1:].var(-1, unbiased=False) + 1e-5).rsqrt().reshape(-1).contiguous()
    dx = torch.zeros(B, 1 + N, D, dtype=torch.bfloat16, device=DEV)
    dg, db = torch.zeros(D, device=DEV), torch.zeros(D, device=DEV)
    ops.layernorm_bwd(dy.to(DEV), D, ops.IDENT, xd, D, tm, B * N, D, mean, rstd, gamma.to(DEV), dres.to(DEV), dx, D, dg, db)
    check('ln_bwd x32 dx', dx.float().cpu(), dx_ref, 1e-2)
    check('ln_bwd x32 dgamma', dg.cpu(), gq.grad, 1e-2)
    check('ln_bwd x32 dbeta', db.cpu(), bq.grad, 1e-2)


def test_timesformer_small_exact_stream_vs_golden():
    """tsf_small divided_space_time, train mode with DropPath draws, against the reference golden: the FIXED bars, and the outputs
    no worse than 1.5 x the reference's own autocast deviation (the default bf16 stream: 1.0 - 2.0 x over the goldens)."""
    import video_transformer as V
    g = gold('tsf_small_divided_space_time.npz')
    m, _ = _build(V.TimeSformer, 3, num_frames=4, attention_type='divided_space_time', **SMALL)
    x = synth.synth_clip(3, 4, 3, 64, 64, seed=2)
    y, grads = _train_step(m, x, 11, 128)
    e = check('tsf_small divided_space_time bf16 exact stream train out', y.cpu(), g['out'], TOL_BF16)
    ref = cal_entry('tsf_small divided_space_time train')['out']
    report(f'     exact stream: out {e:.3e}; reference autocast {ref:.3e}')
    compare_grads('tsf_small divided_space_time bf16 exact stream', grads, g, TOL_BF16_GRAD, cal='tsf_small divided_space_time train', widen=False)
    m.eval()
    with torch.no_grad():
        check('tsf_small divided_space_time bf16 exact stream eval out', m(x.to(DEV)).cpu(), g['out_eval'], TOL_BF16)
        att = m.get_last_selfattention(x.to(DEV))
    check('tsf_small divided_space_time bf16 exact stream last attention', att.cpu(), g['attn'], TOL_BF16)


def test_vivit_small_divided_exact_stream_vs_golden():
    import video_transformer as V
    g = gold('vivit_small_divided_space_time.npz')
    m, _ = _build(V.ViViT, 4, num_frames=8, attention_type='divided_space_time', **SMALL)
    y, grads = _train_step(m, synth.synth_clip(3, 8, 3, 64, 64, seed=5), 13, 128)
    check('vivit_small divided_space_time bf16 exact stream train out', y.cpu(), g['out'], TOL_BF16)
    compare_grads('vivit_small divided_space_time bf16 exact stream', grads, g, TOL_BF16_GRAD, cal='vivit_small divided_space_time train', widen=False)


@pytest.mark.parametrize('at', ['space_only', 'joint_space_time'])
def test_timesformer_small_other_attention_types_exact_stream(at):
    """space_only / joint_space_time (MultiheadAttentionWithPreNorm blocks; space_only's frame mean reads the stream as one
    tensor through StreamValueFn) under the exact stream, fixed bars."""
    import video_transformer as V
    g = gold(f'tsf_small_{at}.npz')
    m, _ = _build(V.TimeSformer, 3, num_frames=4, attention_type=at, **SMALL)
    x = synth.synth_clip(3, 4, 3, 64, 64, seed=2)
    y, grads = _train_step(m, x, 11, 128)
    check(f'tsf_small {at} bf16 exact stream train out', y.cpu(), g['out'], TOL_BF16)
    compare_grads(f'tsf_small {at} bf16 exact stream', grads, g, TOL_BF16_GRAD, cal=f'tsf_small {at} train', widen=False)
    m.eval()
    with torch.no_grad():
        check(f'tsf_small {at} bf16 exact stream eval out', m(x.to(DEV)).cpu(), g['out_eval'], TOL_BF16)
        att = m.get_last_selfattention(x.to(DEV))
    check(f'tsf_small {at} bf16 exact stream last attention', att.cpu(), g['attn'], TOL_BF16)


@pytest.mark.parametrize('at', ['fact_encoder', 'joint_space_time'])
def test_vivit_small_other_attention_types_exact_stream(at):
    """ViViT fact_encoder (two encoders; the glue between them reads the spatial encoder's stream as one tensor, the temporal
    encoder starts a new stream) and joint_space_time under the exact stream, FIXED bars -- fact_encoder is the case on which the
    default bf16 stream has its thinnest gradient margin (worst l2-rel 1.74e-2 against the 2e-2 bar, reference autocast 1.02e-2)."""
    import video_transformer as V
    g = gold(f'vivit_small_{at}.npz')
    m, _ = _build(V.ViViT, 4, num_frames=8, attention_type=at, **SMALL)
    y, grads = _train_step(m, synth.synth_clip(3, 8, 3, 64, 64, seed=5), 13, 128)
    check(f'vivit_small {at} bf16 exact stream train out', y.cpu(), g['out'], TOL_BF16)
    compare_grads(f'vivit_small {at} bf16 exact stream', grads, g, TOL_BF16_GRAD, cal=f'vivit_small {at} train', widen=False)


def test_vivit_b_t16_exact_stream_vs_golden():
    """BASELINE.json configs[2] at full size (ViViT-B fact_encoder, Conv3d tubelets, 16x224^2) under the exact stream: eval forward
    (default bf16 stream: 1.21e-2 where the reference's autocast run deviates by 6.7e-3) and the train step with all gradients."""
    import video_transformer as V
    m, _ = _build(V.ViViT, 0, num_frames=16)
    g = gold('vivit_b_t16_train.npz')
    y, grads = _train_step(m, synth.synth_clip(2, 16, seed=3), 17, 768)
    check('ViViT-B T=16 train bf16 exact stream out', y.cpu(), g['out'], TOL_BF16, cal='ViViT-B T=16 train', widen=False)
    compare_grads('ViViT-B T=16 train bf16 exact stream', grads, g, TOL_BF16_GRAD, cal='ViViT-B T=16 train', widen=False)
    m.eval()
    with torch.no_grad():
        ye = m(synth.synth_clip(2, 16, seed=3).to(DEV))
    e = check('ViViT-B fact_encoder eval bf16 exact stream', ye.cpu(), gold('vivit_b_t16_eval.npz')['out'], TOL_BF16, cal='ViViT-B fact_encoder eval', widen=False)
    assert e <= 1.5 * cal_entry('ViViT-B fact_encoder eval')['out'], f'eval deviation {e:.3e} beyond 1.5 x the reference autocast run'


@pytest.mark.parametrize('mode', ['fp32', 'fp32+grad'])
def test_block_recompute_under_the_exact_stream(mode):
    """vtx.set_recompute(True) with the exact stream: the checkpointed block takes the Stream (contribution, float32 stream) as its
    argument and the re-run in backward gets the same pair -- outputs and gradients bit-identical to the stored-activation run ('fp32+grad': the
    float32 gradient rides on the gradient tensors between the same backward nodes, recompute or not)."""
    import vtx
    import video_transformer as V
    res = []
    try:
        for rc in (False, True):
            vtx.set_recompute(rc)
            vtx.set_stream(mode)
            m, _ = _build(V.TimeSformer, 3, num_frames=4, **SMALL)
            y, grads = _train_step(m, synth.synth_clip(2, 4, 3, 64, 64, seed=2), 11, 128)
            res.append((y.detach().clone(), {k: g.clone() for k, g in grads.items()}))
    finally:
        vtx.set_recompute(False)
    assert torch.equal(res[0][0], res[1][0])
    for k in res[0][1]:
        assert torch.equal(res[0][1][k], res[1][1][k]), k


def test_float32_gradient_stream_survives_only_on_the_unmodified_tensor():
    """The float32 gradient rides on the bf16 gradient tensor as an attribute with that tensor's version counter: a second consumer of
    a block's output makes autograd ACCUMULATE into the tensor (in place: the version moves; out of place: another object) -- the
    stale float32 buffer must then be dropped and the stream's gradient restarted from the accumulated bf16 tensor."""
    import vtx
    from vtx import functions as F_
    vtx.set_stream('fp32+grad')
    d = torch.randn(2, 5, 128, device=DEV).bfloat16()
    xs = torch.randn(2, 5, 128, device=DEV)
    g32 = torch.randn(2, 5, 128, device=DEV)
    d._vtx_g32 = (g32, d._version)
    assert F_._grad_stream(d, xs) is g32
    d.add_(1)                                                    # what InputBuffer::add does to the first gradient
    fresh = F_._grad_stream(d, xs)
    assert fresh is not g32 and torch.equal(fresh, d.float())
    assert F_._grad_stream(d.clone(), xs) is not g32               # another object: no attribute
    vtx.set_stream('fp32')
    assert F_._grad_stream(d, xs) is None                        # mode off
    # end to end: a tap on the stream between two blocks (a second consumer) still gives the right gradients
    import transformer as T_
    import video_transformer as V
    grads = {}
    for mode in ('fp32', 'fp32+grad'):
        vtx.set_stream(mode)
        m, _ = _build(V.TimeSformer, 3, num_frames=4, **SMALL)
        m.train(); m.zero_grad()
        taps = []
        h = m.transformer_layers.layers[1].register_forward_hook(lambda mod, inp, out: taps.append(out))
        torch.manual_seed(11)
        y = m(synth.synth_clip(2, 4, 3, 64, 64, seed=2).to(DEV))
        h.remove()
        (y.float().sum() + 0.5 * T_.stream_value(taps[0]).float().sum()).backward()
        grads[mode] = {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}
    for k in grads['fp32']:
        e = relerr(grads['fp32+grad'][k].cpu(), grads['fp32'][k].cpu())
        assert e < 2e-2, (k, e)


def test_timesformer_b_t8_exact_stream_vs_golden_and_reference_autocast():
    """BASELINE.json configs[1] (TimeSformer-B 8x224^2, train mode with DropPath) under the exact stream: fixed bars on outputs and
    all 247 gradients, the eval forward, and the attention-map slice at the FIXED 1.5e-2 (the default bf16 stream needs a bar
    calibrated against the reference under a bf16 stream there: tests/test_gpu_00_baseline_configs.py)."""
    import video_transformer as V
    g = gold('tsf_b_t8_autocast.npz')
    m, _ = _build(V.TimeSformer, 0, num_frames=8)
    y, grads = _train_step(m, synth.synth_clip(1, 8, seed=1), 7, 768)
    e = check('TimeSformer-B T=8 train bf16 exact stream out', y.cpu(), g['out'], TOL_BF16)
    report(f'     exact stream: out {e:.3e}; reference autocast {relerr(g["out_autocast"], g["out"]):.3e}')
    compare_grads('TimeSformer-B T=8 train bf16 exact stream', grads, g, TOL_BF16_GRAD, autocast_cal=True)
    ge = gold('tsf_b_t8_eval.npz')
    m.eval()
    with torch.no_grad():
        x = synth.synth_clip(1, 8, seed=1).to(DEV)
        check('TimeSformer-B T=8 eval bf16 exact stream out', m(x).cpu(), ge['out'], TOL_BF16)
        att = m.get_last_selfattention(x)
    c = cal_entry('TimeSformer-B T=8 attention')
    e = check('TimeSformer-B T=8 bf16 exact stream attention', att[:2, :, :8, :8].cpu(), ge['attn_head'], TOL_BF16)
    report(f'     exact stream: attention slice {e:.3e}; reference autocast {c["out"]:.3e}, reference autocast with a bf16 stream {c["out_bf16_stream"]:.3e}')


def test_timesformer_l_t96_full_depth_exact_stream():
    """BASELINE.json configs[4] at full depth (24 layers, 18 817 tokens) under the exact stream: the FIXED 1.5e-2 bar, and within
    2 x the reference's own autocast deviation (5.0e-3) -- where the default bf16 stream measures 1.2 - 1.6e-2."""
    import video_transformer as V
    g = gold('tsf_l_t96_d24_eval.npz')
    m, _ = _build(V.TimeSformer, 0, num_frames=96, embed_dims=1024, num_heads=16, num_transformer_layers=24)
    m.eval()
    with torch.no_grad():
        y = m(synth.synth_clip(1, 96, seed=5).to(DEV))
    del m
    torch.cuda.empty_cache()
    ref_ac = relerr(g['out_autocast'], g['out'])
    e = check('TimeSformer-L T=96 depth 24 eval bf16 exact stream out', y.cpu(), g['out'], TOL_BF16)
    report(f'     exact stream: {e:.3e}; reference autocast {ref_ac:.3e}; reference autocast with a bf16 stream {relerr(g["out_autocast_bf16_stream"], g["out"]):.3e}')
    assert e <= 2.0 * ref_ac, f'exact stream {e:.3e} > 2 x the reference autocast deviation {ref_ac:.3e}'


@pytest.mark.parametrize('mode', ['fp32', 'fp32+grad'])
def test_bench_stack_exact_stream_with_partial_ffn_drop(mode):
    """The bench stack (direct gradients into buckets, DropPath compaction with some clips of a layer dropped, merged projection)
    under the exact stream against the oracle at 8 clips: the dropped clips' stream rows move on through the accumulate-only
    kernel, their contribution rows are zero ('fp32+grad': their float32 gradient rows pass through the block as they came)."""
    import vtx
    import video_transformer as V
    vtx.set_stream(mode)
    from vtx import dp
    from test_gpu_models import _ffn_drop_pattern
    B, T, L = 8, 16, 4
    cfg = dict(img_size=64, patch_size=16, embed_dims=128, num_heads=2, num_transformer_layers=L)
    P = (64 // 16) ** 2
    seed = next(s for s in range(200) if any(0 < sum(l) < B for l in _ffn_drop_pattern(s, B, P, T, L)))
    m, sd = _build(V.TimeSformer, 5, num_frames=T, **cfg)
    x = synth.synth_clip(B, T, 3, 64, 64, seed=4)
    w = synth_tensor('loss_w', (128,), 0) * 10.0
    buckets = dp.GradBuckets(list(m.parameters()), bucket_bytes=256 << 10, direct=True)
    try:
        buckets.zero()
        m.train()
        torch.manual_seed(seed)
        y = m(x.to(DEV))
        (y * w.to(DEV)).sum().backward()
        buckets.finish()
        torch.cuda.synchronize()
        grads = {k: p.grad.detach().cpu().clone() for k, p in m.named_parameters()}
    finally:
        buckets.remove()
    ps = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    torch.manual_seed(seed)
    yo = O.timesformer_forward(ps, x, T, heads=2, layers=L, training=True)
    (yo * w).sum().backward()
    check(f'bench stack bf16 exact stream {mode} out', y.detach().cpu(), yo.detach(), TOL_BF16)
    worst = 0.0
    for k, gk in grads.items():
        ref = ps[k].grad
        e = (gk.double() - ref.double()).norm().item() / max(ref.double().norm().item(), 1e-30)
        worst = max(worst, e)
        assert e <= TOL_BF16_GRAD, f'{k}: {e:.3e}'
    report(f'bench stack bf16 exact stream {mode}: worst parameter gradient l2-rel {worst:.3e}')


# ---- the hand-off between sub-blocks: transformer.Stream(d, xs) ----------------------------------------------------------------
# The smallest model that has every hand-off (tokens -> block, attention -> attention -> FFN, block -> block, block -> readout).

def _handoff_model(at='divided_space_time'):
    import video_transformer as V
    m, _ = _build(V.TimeSformer, 3, num_frames=4, attention_type=at, **dict(SMALL, num_transformer_layers=3))
    return m.eval(), synth.synth_clip(2, 4, 3, 64, 64, seed=2).to(DEV)


@pytest.mark.parametrize('at', ['divided_space_time', 'space_only', 'joint_space_time'])
@pytest.mark.parametrize('mode', ['fp32', 'fp32+grad', 'bf16', 'fp32 under float32 compute'])
def test_what_the_sub_blocks_hand_on(at, mode):
    """Every sub-block, every block and the container hand on a Stream (bf16 contribution, float32 stream of the same shape) in the
    two exact modes under bf16 compute, and a plain tensor otherwise (mode off; float32 compute is its own exact stream)."""
    import vtx
    import transformer as T_
    exact = mode in ('fp32', 'fp32+grad')
    if mode == 'fp32 under float32 compute':
        vtx.set_precision('fp32')
    vtx.set_stream(mode if exact or mode == 'bf16' else 'fp32')
    m, clip = _handoff_model(at)
    outs, hooks = [], []
    mods = [m.transformer_layers] + list(m.transformer_layers.layers)
    mods += [sub for blk in m.transformer_layers.layers for sub in list(blk.attentions) + list(blk.ffns)]
    for mod in mods:
        hooks.append(mod.register_forward_hook(lambda mod, inp, out: outs.append(out)))
    with torch.no_grad():
        y = m(clip)
    for h in hooks:
        h.remove()
    n_sub = 3 if at == 'divided_space_time' else 2
    assert len(outs) == 1 + 3 + 3 * n_sub and y.dtype == torch.float32
    for out in outs:
        if exact:
            assert type(out) is T_.Stream
            assert out.d.dtype == torch.bfloat16 and out.xs.dtype == torch.float32 and out.xs.shape == out.d.shape
            assert not out.xs.requires_grad
        else:
            assert type(out) is torch.Tensor


def test_stream_value_is_the_rounded_sum():
    """stream_value(Stream(d, xs)) = bf16(xs + d): one round-to-nearest-even of the float32 sum (that the kernel's sum IS the
    float32 sum: test_layernorm_acc_fwd_vs_float64)."""
    import transformer as T_
    m, clip = _handoff_model()
    with torch.no_grad():
        s = m.transformer_layers(m.prepare_tokens(clip)[0])
        assert type(s) is T_.Stream
        assert torch.equal(T_.stream_value(s), (s.xs + s.d.float()).to(torch.bfloat16))


def test_the_readout_takes_the_pair():
    import transformer as T_
    m, clip = _handoff_model()
    with torch.no_grad():
        s = m.transformer_layers(m.prepare_tokens(clip)[0])
        assert type(s) is T_.Stream
        assert torch.equal(m._readout(s), m(clip))


def test_a_collapsed_stream_restarts_instead_of_vanishing():
    """A forward hook that turns a block's output into one tensor (stream_value): the next block starts a new stream AT that
    tensor -- the whole sum up to there, not the last contribution alone.  Bit-equal to block 2 and the readout run by hand on it."""
    import transformer as T_
    m, clip = _handoff_model()
    seen = []

    def collapse(mod, inp, out):
        seen.append(T_.stream_value(out))
        return seen[-1]
    h = m.transformer_layers.layers[1].register_forward_hook(collapse)
    with torch.no_grad():
        y = m(clip)
        h.remove()
        assert len(seen) == 1 and type(seen[0]) is torch.Tensor and seen[0].dtype == torch.bfloat16
        by_hand = m._readout(m.transformer_layers.layers[2](seen[0]))
    assert torch.equal(y, by_hand)


# ---- 'fp32+grad': the stream's gradient in float32 too ---------------------------------------------------------------------

def test_layernorm_bwd_g32_vs_float64():
    """vtx_layernorm_bwd_g32: dx32 = dres32 + LayerNorm-backward(dy) in float32 on the mapped rows, dx = bf16(dx32) EXACTLY (one
    rounding of the float32 sum), dgamma / dbeta as vtx_layernorm_bwd; rows outside the map untouched."""
    from vtx import ops
    for D in (128, 200, 768, 1024):
        B, N = 3, 37
        x = (rnd(B, 1 + N, D, seed=1) * 2 + 0.5)
        gamma = 1 + 0.1 * rnd(D, seed=2)
        dy = rnd(B * N, D, seed=4).bfloat16()
        dres32 = rnd(B, 1 + N, D, seed=5) * 3
        xq = x.double().requires_grad_(True)
        gq, bq = gamma.double().requires_grad_(True), torch.zeros(D, dtype=torch.float64, requires_grad=True)
        ref = torch.nn.functional.layer_norm(xq[:, 1:], (D,), gq, bq, 1e-5).reshape(B * N, D)
        ref.backward(dy.double())
        dx_ref = xq.grad + dres32.double()
        tm = ops.tokmap(N)
        xd = x.to(DEV)
        mean = xd[:, 1:].mean(-1).reshape(-1).contiguous()
        rstd = (xd[:, 1:].var(-1, unbiased=False) + 1e-5).rsqrt().reshape(-1).contiguous()
        dx = torch.full((B, 1 + N, D), 7.0, dtype=torch.bfloat16, device=DEV)
        dx32 = torch.full((B, 1 + N, D), 7.0, device=DEV)
        dg, db = torch.zeros(D, device=DEV), torch.zeros(D, device=DEV)
        ops.layernorm_bwd(dy.to(DEV), D, ops.IDENT, xd, D, tm, B * N, D, mean, rstd, gamma.to(DEV), None, dx, D, dg, db,
                          dres32=dres32.to(DEV), dx32=dx32)
        torch.cuda.synchronize()
        check(f'ln_bwd_g32 dx32 D={D}', dx32[:, 1:].cpu(), dx_ref[:, 1:], 1e-5)
        assert torch.equal(dx[:, 1:].cpu(), dx32[:, 1:].bfloat16().cpu()), 'dx is the single rounding of the float32 sum'
        assert bool((dx32[:, 0] == 7).all()) and bool((dx[:, 0] == 7).all()), 'the cls rows are outside the token map'
        check(f'ln_bwd_g32 dgamma D={D}', dg.cpu(), gq.grad, 1e-2)
        check(f'ln_bwd_g32 dbeta D={D}', db.cpu(), bq.grad, 1e-2)


def _grads_of(V, cls, nblk, at, x, seed, stream, **kw):
    import vtx
    vtx.set_stream(stream)
    m, _ = _build(cls, nblk, attention_type=at, **kw)
    return _train_step(m, x, seed, 128)


@pytest.mark.parametrize('case', ['tsf divided_space_time', 'tsf joint_space_time', 'vivit fact_encoder', 'vivit divided_space_time'])
def test_float32_gradient_stream_vs_golden(case):
    """vtx.set_stream('fp32+grad') against the reference goldens with the FIXED bars: outputs bit-identical to 'fp32' (the forward is
    the same), the gradients no worse at the median than under 'fp32'; the gradient of the FIRST tensors of the backward chain (patch
    embedding, position embedding: they see the whole stream's gradient) closer to the reference than with the bf16 gradient stream."""
    import vtx
    import video_transformer as V
    fam, at = case.split()
    if fam == 'tsf':
        cls, nblk, x, seed, kw, gname = V.TimeSformer, 3, synth.synth_clip(3, 4, 3, 64, 64, seed=2), 11, dict(num_frames=4, **SMALL), f'tsf_small_{at}'
    else:
        cls, nblk, x, seed, kw, gname = V.ViViT, 4, synth.synth_clip(3, 8, 3, 64, 64, seed=5), 13, dict(num_frames=8, **SMALL), f'vivit_small_{at}'
    g = gold(gname + '.npz')
    y1, g1 = _grads_of(V, cls, nblk, at, x, seed, 'fp32', **kw)
    y2, g2 = _grads_of(V, cls, nblk, at, x, seed, 'fp32+grad', **kw)
    assert vtx.get_stream() == 'fp32+grad'
    assert torch.equal(y1, y2), 'the forward does not depend on the gradient stream'
    c1, c2 = {}, {}
    cal = f'{gname.replace("_small_", "_small ")} train'
    compare_grads(f'{gname} bf16 exact stream (again)', g1, g, TOL_BF16_GRAD, cal=cal, widen=False, collect=c1)
    compare_grads(f'{gname} bf16 exact stream + float32 gradient stream', g2, g, TOL_BF16_GRAD, cal=cal, widen=False, collect=c2)
    e1, e2 = [c1[k] for k in c1], [c2[k] for k in c1]
    med = lambda v: sorted(v)[len(v) // 2]      # noqa: E731
    report(f'     {case}: median / worst gradient l2-rel  fp32 stream {med(e1):.3e} / {max(e1):.3e}   + float32 gradient stream {med(e2):.3e} / {max(e2):.3e}'
           f'   ({sum(b < a for a, b in zip(e1, e2))} of {len(e1)} tensors closer to the reference)')
    assert med(e2) <= 1.10 * med(e1), (med(e1), med(e2))      # 3 - 4 layers: the two gradient streams differ by rounding noise only


@pytest.mark.parametrize('case', ['TimeSformer-B T=8', 'ViViT-B T=16'])
def test_float32_gradient_stream_full_size(case):
    """BASELINE configs[1] / [2] at full size (12 layers: 36 / 32 sub-blocks of gradient stream) under 'fp32+grad': every gradient
    inside the FIXED bars, the median no worse than under 'fp32', and the report carries both modes next to the reference's autocast."""
    import vtx
    import video_transformer as V
    if case.startswith('Time'):
        g, build, x, seed = gold('tsf_b_t8_autocast.npz'), (lambda: _build(V.TimeSformer, 0, num_frames=8)[0]), synth.synth_clip(1, 8, seed=1), 7
    else:
        g, build, x, seed = gold('vivit_b_t16_train.npz'), (lambda: _build(V.ViViT, 0, num_frames=16)[0]), synth.synth_clip(2, 16, seed=3), 17
    c = {}
    for mode in ('fp32', 'fp32+grad'):
        vtx.set_stream(mode)
        y, grads = _train_step(build(), x, seed, 768)
        check(f'{case} train bf16 stream {mode} out', y.cpu(), g['out'], TOL_BF16)
        c[mode] = {}
        kw = dict(autocast_cal=True) if case.startswith('Time') else dict(cal='ViViT-B T=16 train', widen=False)
        compare_grads(f'{case} train bf16 stream {mode}', grads, g, TOL_BF16_GRAD, collect=c[mode], **kw)
    e1, e2 = [c['fp32'][k] for k in c['fp32']], [c['fp32+grad'][k] for k in c['fp32']]
    med = lambda v: sorted(v)[len(v) // 2]      # noqa: E731
    report(f'     {case}: median / worst gradient l2-rel  fp32 stream {med(e1):.3e} / {max(e1):.3e}   + float32 gradient stream {med(e2):.3e} / {max(e2):.3e}'
           f'   ({sum(b < a for a, b in zip(e1, e2))} of {len(e1)} tensors closer to the reference)')
    assert med(e2) <= 1.03 * med(e1), (med(e1), med(e2))
