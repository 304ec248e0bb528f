"""Mixup / CutMix on decoded uint8 clips (csrc/mix.hip, vtx.ops.cutmix_batch_u8_, vtx.MixedClip, mixup.Mixup on uint8): the
box swap byte for byte with guard bytes around an unaligned clip, the mixed patch rows bit for bit against the reference's
arithmetic restated with torch on the CPU and against the existing float route on the device, Mixup's draw and targets on
uint8 against the float call, and the path through TimeSformer and ViViT."""
import numpy as np
import pytest
import torch

from model_common import DEV, _build, _reset_precision  # noqa: F401

pytestmark = pytest.mark.gpu

MEAN, STD = [0.45, 0.456, 0.406], [0.225, 0.224, 0.229]


def _normalised(u8):
    """ToTensor + Normalize of the reference on a uint8 [B,T,H,W,3] clip -> float [B,T,3,H,W] (as
    tests/test_gpu_kernels.py::test_patch_rows_uint8_ingest_bit_exact restates them)."""
    x = u8.permute(0, 1, 4, 2, 3).float().div(255)
    return x.sub(torch.tensor(MEAN).view(1, 1, 3, 1, 1)).div(torch.tensor(STD).view(1, 1, 3, 1, 1)).contiguous()


def _every_byte_clip(B, T, H, W, seed):
    """Random bytes in which every value 0..255 occurs in every clip -- so in both partners of every pair."""
    g = torch.Generator().manual_seed(seed)
    u8 = torch.randint(0, 256, (B, T, H, W, 3), generator=g, dtype=torch.uint8)
    assert T * H * W * 3 >= 2 * 256
    for b in range(B):
        flat = u8[b].view(-1)
        flat[b:b + 256] = torch.arange(256, dtype=torch.uint8)
        flat[-256 - b:flat.numel() - b] = torch.arange(255, -1, -1, dtype=torch.uint8)
        assert len(torch.unique(u8[b])) == 256
    return u8


# ------------------------------------------------------------------------------------------------ CutMix
BOXES = {'full': None, 'one-pixel': (3, 4, 2, 3), 'inner': (2, 9, 1, 6), 'two-borders': (0, 6, 3, 7), 'empty': (4, 4, 1, 6)}


def _swap_reference(u8, box):
    """mixup.py:109 on the [B,T,3,H,W] permutation of the clip: x[:, :, yl:yh, xl:xh] = x.flip(0)[:, :, yl:yh, xl:xh]."""
    yl, yh, xl, xh = box
    x = u8.permute(0, 1, 4, 2, 3).clone()
    x[..., yl:yh, xl:xh] = x.flip(0)[..., yl:yh, xl:xh]
    return x.permute(0, 1, 3, 4, 2).contiguous()


def _guarded(u8, lead):
    """The clip as a slice `lead` bytes into a larger device buffer with sentinel bytes on both sides."""
    n = u8.numel()
    buf = torch.full((lead + n + 64,), 0xA5, dtype=torch.uint8)
    buf[lead:lead + n] = u8.view(-1)
    buf = buf.to(DEV)
    return buf, buf[lead:lead + n].view(u8.shape)


@pytest.mark.parametrize('B', [2, 4])
@pytest.mark.parametrize('box', list(BOXES), ids=list(BOXES))
def test_cutmix_u8_swaps_the_box_bytes_and_nothing_else(B, box):
    """21-byte rows, a clip one byte off every alignment, 420 bytes between the clips of the inner pair: no piece of any box
    row is aligned in both partners (the byte path).  The result is the reference's assignment, the guard bytes and every byte
    outside the box are unchanged, and a second call restores the clip."""
    from vtx import ops
    T, H, W = 2, 10, 7
    g = torch.Generator().manual_seed(5)
    u8 = torch.randint(0, 256, (B, T, H, W, 3), generator=g, dtype=torch.uint8)
    bx = BOXES[box] or (0, H, 0, W)
    want = _swap_reference(u8, bx)
    buf, clip = _guarded(u8, 1)
    assert clip.data_ptr() % 2 == 1 and clip.is_contiguous()
    out = ops.cutmix_batch_u8_(clip, *bx)
    assert out is clip
    got = buf.cpu()
    n = u8.numel()
    assert torch.equal(got[1:1 + n].view(u8.shape), want), f'{box}: swapped clip differs'
    assert (got[:1] == 0xA5).all() and (got[1 + n:] == 0xA5).all(), f'{box}: guard bytes written'
    if box == 'empty':
        assert torch.equal(want, u8)
    else:
        assert not torch.equal(want, u8)
    ops.cutmix_batch_u8_(clip, *bx)
    assert torch.equal(buf.cpu()[1:1 + n].view(u8.shape), u8), f'{box}: the second swap does not restore the clip'


@pytest.mark.parametrize('lead', [0, 16, 3])
@pytest.mark.parametrize('B', [2, 4])
def test_cutmix_u8_wide_path(B, lead):
    """32x32 frames (96-byte rows, 6144 bytes per clip): with an aligned box every piece moves as 16 bytes, with an unaligned
    one the row ends move as bytes around 16-byte pieces, and with the clip 3 bytes off both partners are misaligned alike."""
    from vtx import ops
    T, H, W = 2, 32, 32
    g = torch.Generator().manual_seed(6)
    u8 = torch.randint(0, 256, (B, T, H, W, 3), generator=g, dtype=torch.uint8)
    n = u8.numel()
    for bx in ((8, 24, 16, 32), (0, 32, 0, 32), (5, 30, 3, 30)):
        want = _swap_reference(u8, bx)
        buf, clip = _guarded(u8, lead)
        ops.cutmix_batch_u8_(clip, *bx)
        got = buf.cpu()
        assert torch.equal(got[lead:lead + n].view(u8.shape), want), f'{bx}: swapped clip differs'
        assert (got[:lead] == 0xA5).all() and (got[lead + n:] == 0xA5).all(), f'{bx}: guard bytes written'
        ops.cutmix_batch_u8_(clip, *bx)
        assert torch.equal(buf.cpu()[lead:lead + n].view(u8.shape), u8), f'{bx}: the second swap does not restore the clip'


def test_cutmix_u8_rejects_what_it_cannot_take():
    from vtx import ops
    from vtx._lib import VtxError
    clip = torch.zeros(2, 2, 10, 7, 3, dtype=torch.uint8, device=DEV)
    with pytest.raises(TypeError):
        ops.cutmix_batch_u8_(clip.float(), 0, 1, 0, 1)
    with pytest.raises(TypeError):
        ops.cutmix_batch_u8_(clip[..., :2], 0, 1, 0, 1)
    with pytest.raises(VtxError, match='outside'):
        ops.cutmix_batch_u8_(clip, 0, 11, 0, 1)
    with pytest.raises(VtxError, match='even'):
        ops.cutmix_batch_u8_(torch.zeros(3, 2, 10, 7, 3, dtype=torch.uint8, device=DEV), 0, 1, 0, 1)


# ------------------------------------------------------------------------------------------------ mixed rows
LAMS = {'0.3': 0.3, '0.1': 0.1, 'beta': float(np.random.RandomState(20261019).beta(0.8, 0.8)), '1e-8': 1e-8}
assert float(np.float32(1. - LAMS['0.1'])) != 1. - float(np.float32(LAMS['0.1']))     # 1 - lam is formed in float64, then rounded once
SHAPES = {'ps16': (16, 32, 48), 'ps4': (4, 8, 12)}
_shared = {}


def _mix_case(B, shape, lam_id):
    """The uint8 clip, and the reference's Mixup of its normalised float form -- computed once per case, on the CPU."""
    key = (B, shape, lam_id)
    if key not in _shared:
        ps, H, W = SHAPES[shape]
        T = 4
        u8 = _every_byte_clip(B, T, H, W, seed=3 + B)
        lam = LAMS[lam_id]
        x = _normalised(u8)
        planes = x.view(B, -1, H, W)                                     # mixup.py:104-113 on the [B,T*C,H,W] view
        x_flipped = planes.flip(0).mul_(1. - lam)
        planes.mul_(lam).add_(x_flipped)
        _shared[key] = (u8, x)
    return _shared[key]


def _oracle_rows(x, ps, ts, frame_major):
    from oracle import vt_oracle as O
    B, T = x.shape[:2]
    Tq = T // ts
    want = O.patch_rows_2d(x, ps) if ts == 1 else O.patch_rows_3d(x, ps, ts)      # [(B Tq), P, K]
    P, K = want.shape[1], want.shape[2]
    if frame_major:
        return want.reshape(B * Tq * P, K)
    return want.reshape(B, Tq, P, K).permute(0, 2, 1, 3).reshape(B * P * Tq, K)


@pytest.mark.parametrize('lam_id', list(LAMS))
@pytest.mark.parametrize('shape', list(SHAPES))
@pytest.mark.parametrize('ts', [1, 2])
@pytest.mark.parametrize('B', [2, 4])
def test_mixed_rows_bit_exact(B, ts, shape, lam_id):
    """vtx_patch_rows_mix_u8 through ops.patch_rows(MixedClip): fp32 rows torch.equal to ToTensor, Normalize, the reference's
    flip / mul_ / add_ and the oracle's gather on the CPU; bf16 rows equal to those rounded once; both equal to the existing
    device route (ops.mixup_batch_ then ops.patch_rows on the float clip); both row orders; the clip is not modified."""
    import vtx
    from vtx import ops
    ps, H, W = SHAPES[shape]
    lam = LAMS[lam_id]
    u8, mixed = _mix_case(B, shape, lam_id)
    clip = u8.to(DEV)
    carrier = vtx.MixedClip(clip, lam)
    assert carrier.shape == clip.shape and carrier.device == clip.device and carrier.dtype == torch.uint8 and len(carrier) == B
    assert ops.clip_dims(carrier) == (B, 4, 3, H, W)
    xf = _normalised(u8).to(DEV)
    ops.mixup_batch_(xf.view(B, -1, H, W), lam)
    vtx.set_input_normalization(MEAN, STD)
    try:
        for frame_major in (True, False):
            want = _oracle_rows(mixed, ps, ts, frame_major)
            got = ops.patch_rows(carrier, torch.float32, ps, ts, frame_major=frame_major)
            assert got.shape == want.shape and torch.equal(got.cpu(), want), f'fp32 rows differ (frame_major={frame_major})'
            assert torch.equal(got, ops.patch_rows(xf, torch.float32, ps, ts, frame_major=frame_major)), 'fp32 rows differ from the float route'
            got16 = ops.patch_rows(carrier, torch.bfloat16, ps, ts, frame_major=frame_major)
            assert torch.equal(got16.cpu(), want.to(torch.bfloat16)), f'bf16 rows differ from the rounded fp32 rows (frame_major={frame_major})'
            assert torch.equal(got16, ops.patch_rows(xf, torch.bfloat16, ps, ts, frame_major=frame_major)), 'bf16 rows differ from the float route'
    finally:
        vtx.set_input_normalization(None, None)
    assert torch.equal(clip.cpu(), u8), 'the uint8 clip was modified'
    with pytest.raises(ValueError, match='set_input_normalization'):
        ops.patch_rows(carrier, torch.float32, ps, ts, frame_major=True)


def test_mixed_rows_with_narrow_stores():
    """ps = 12 is a multiple of 4 and not of 8: the four-pixel path of the kernel at a patch size whose runs are 36 bytes."""
    import vtx
    from vtx import ops
    B, T, H, W, ps, lam = 2, 2, 24, 36, 12, 0.3
    u8 = _every_byte_clip(B, T, H, W, seed=9)
    x = _normalised(u8)
    planes = x.view(B, -1, H, W)
    x_flipped = planes.flip(0).mul_(1. - lam)
    planes.mul_(lam).add_(x_flipped)
    vtx.set_input_normalization(MEAN, STD)
    try:
        for frame_major in (True, False):
            want = _oracle_rows(x, ps, 1, frame_major)
            got = ops.patch_rows(vtx.MixedClip(u8.to(DEV), lam), torch.float32, ps, 1, frame_major=frame_major)
            assert torch.equal(got.cpu(), want)
            got16 = ops.patch_rows(vtx.MixedClip(u8.to(DEV), lam), torch.bfloat16, ps, 1, frame_major=frame_major)
            assert torch.equal(got16.cpu(), want.to(torch.bfloat16))
    finally:
        vtx.set_input_normalization(None, None)


# ------------------------------------------------------------------------------------------------ mixup.Mixup
#: np.random seed -> what Mixup(prob=0.6).draw makes of a 32x48 frame
DRAWS = {'mixup': (0, None), 'cutmix': (11, (2, 24, 11, 45)), 'nothing': (4, None)}


@pytest.mark.parametrize('kind', list(DRAWS))
def test_mixup_on_uint8_equals_mixup_on_float(kind):
    """The same seeded call on the bytes and on the normalised float clip: the same soft targets, the same np.random state
    afterwards, and the same patch rows.  H = 32, W = 48: a box drawn from the channels-last tensor's last two dimensions
    (48, 3) would show."""
    import vtx
    from mixup import Mixup
    from vtx import ops
    seed, box = DRAWS[kind]
    B, T, H, W, ps = 4, 4, 32, 48, 16
    u8 = _every_byte_clip(B, T, H, W, seed=21)
    labels = torch.tensor([1, 4, 0, 2], device=DEV)
    fn = Mixup(prob=0.6, num_classes=5)
    np.random.seed(seed)
    lam, drawn = fn.draw((B, T * 3, H, W))
    assert drawn == box and (lam == 1.) == (kind == 'nothing'), f'seed {seed} no longer draws {kind}'

    xf = _normalised(u8).to(DEV)
    np.random.seed(seed)
    yf, tf = fn(xf, labels)
    state_f = np.random.get_state()
    clip = u8.to(DEV)
    np.random.seed(seed)
    y8, t8 = fn(clip, labels)
    state_8 = np.random.get_state()

    assert torch.equal(t8, tf) and t8.shape == (B, 5)
    assert state_8[0] == state_f[0] and np.array_equal(state_8[1], state_f[1]) and state_8[2:] == state_f[2:]
    if kind == 'mixup':
        assert isinstance(y8, vtx.MixedClip) and y8.clip is clip and y8.lam == lam and torch.equal(clip.cpu(), u8)
    elif kind == 'cutmix':
        assert y8 is clip and torch.equal(clip.cpu(), _swap_reference(u8, box)) and not torch.equal(clip.cpu(), u8)
    else:
        assert y8 is clip and torch.equal(clip.cpu(), u8)
    vtx.set_input_normalization(MEAN, STD)
    try:
        for dtype in (torch.float32, torch.bfloat16):
            assert torch.equal(ops.patch_rows(y8, dtype, ps, 1, frame_major=False), ops.patch_rows(yf, dtype, ps, 1, frame_major=False))
    finally:
        vtx.set_input_normalization(None, None)


def test_mixup_uint8_odd_batch_and_wrong_layout_raise():
    from mixup import Mixup
    fn = Mixup(num_classes=5)
    with pytest.raises(AssertionError, match='even'):
        fn(torch.zeros(3, 4, 32, 48, 3, dtype=torch.uint8, device=DEV), torch.zeros(3, dtype=torch.long, device=DEV))
    with pytest.raises(ValueError, match=r'\[B,T,H,W,3\]'):
        fn(torch.zeros(2, 4, 3, 32, 48, dtype=torch.uint8, device=DEV), torch.zeros(2, dtype=torch.long, device=DEV))


# ------------------------------------------------------------------------------------------------ models
TINY = dict(img_size=32, patch_size=16, embed_dims=128, num_heads=2, num_transformer_layers=1)
MODELS = {
    'timesformer-divided': ('TimeSformer', dict(num_frames=4, attention_type='divided_space_time')),
    'timesformer-space-only': ('TimeSformer', dict(num_frames=4, attention_type='space_only')),
    'timesformer-joint': ('TimeSformer', dict(num_frames=4, attention_type='joint_space_time')),
    'vivit-fact-tubelets': ('ViViT', dict(num_frames=4, tube_size=2, attention_type='fact_encoder')),
    'vivit-joint-tubelets': ('ViViT', dict(num_frames=4, tube_size=2, attention_type='joint_space_time')),
    'vivit-divided-tubelets': ('ViViT', dict(num_frames=4, tube_size=2, attention_type='divided_space_time')),
}


@pytest.mark.parametrize('prec', ['fp32', 'bf16'])
@pytest.mark.parametrize('name', list(MODELS), ids=list(MODELS))
def test_model_on_mixed_clip_equals_model_on_float_mixed_clip(name, prec):
    """model(MixedClip(u8, lam)) against model(the float batch the reference's Mixup makes of the normalised clip): the
    outputs and the gradient of the patch projection's weight are torch.equal, in training mode with a backward."""
    import vtx
    import video_transformer as V
    cls, kw = MODELS[name]
    lam = 0.3
    u8, mixed = _mix_case(2, 'ps16', '0.3')
    u8, mixed = u8[..., :32, :].contiguous(), mixed[..., :32].contiguous()       # 32x32 frames of the shared 32x48 case
    vtx.set_precision(prec)
    m, _ = _build(getattr(V, cls), 5, **kw, **TINY)
    m.train()
    vtx.set_input_normalization(MEAN, STD)
    try:
        outs = []
        for inp in (vtx.MixedClip(u8.to(DEV), lam), mixed.to(DEV)):
            m.zero_grad()
            torch.manual_seed(1)
            y = m(inp)
            y.sum().backward()
            outs.append((y.detach().clone(), m.patch_embed.projection.weight.grad.clone()))
        with torch.no_grad():
            m.eval()
            a8 = m.get_last_selfattention(vtx.MixedClip(u8.to(DEV), lam))
            af = m.get_last_selfattention(mixed.to(DEV))
    finally:
        vtx.set_input_normalization(None, None)
    (y8, g8), (yf, gf) = outs
    assert y8.shape[0] == 2 and torch.isfinite(y8).all() and g8.abs().max() > 0
    assert torch.equal(y8, yf), f'{name} {prec}: outputs differ'
    assert torch.equal(g8, gf), f'{name} {prec}: patch projection weight gradients differ'
    assert type(a8) is type(af) and all(torch.equal(p, q) for p, q in zip(*[(a,) if torch.is_tensor(a) else tuple(a) for a in (a8, af)])), \
        f'{name} {prec}: last self-attention differs'


def test_mvit_refuses_a_mixed_clip():
    """MViT's im2col stem is out of scope: a MixedClip raises a TypeError that says so, at the stem and through MaskFeat."""
    import mvit
    import vtx
    carrier = vtx.MixedClip(torch.zeros(2, 4, 32, 32, 3, dtype=torch.uint8, device=DEV), 0.3)
    stem = mvit.create_conv_patch_embed(in_channels=3, out_channels=16).to(DEV)
    with pytest.raises(TypeError, match='MixedClip'):
        stem(carrier)
