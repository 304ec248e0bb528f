"""MaskFeat from decoded uint8 clips (csrc/stem.hip -> libvtx_stem.so; ops.im2col3d_u8, vtx.hog_targets, ConvStemFn / PatchEmbeding /
MaskFeat on uint8): the stem gather bit for bit against vtx_im2col3d of the normalised float clip and against pad + unfold on the
CPU, the stem and the model on bytes against the same call on the normalised float clip, the HOG targets against hog_fwd of the
gathered centre frames and the CPU oracle.  Every comparison is equality; bit patterns are compared where the sign of a zero
matters."""
import ctypes

import numpy as np
import pytest
import torch

import exact_pool as P
from model_common import DEV, _reset_precision  # noqa: F401

pytestmark = pytest.mark.gpu

MEAN, STD = [0.45, 0.456, 0.406], [0.225, 0.224, 0.229]      # ImageNet-style: n(0, c) = -mean / std is far from 0
F32, BF16 = torch.float32, torch.bfloat16
TDT = {'f32': F32, 'bf16': BF16}
BITS = {F32: torch.int32, BF16: torch.int16}
TAIL = 2                                                       # guard rows behind the M rows
I3 = ctypes.c_int * 3

# (k3, s3, p3, (B, T, H, W), Kp)
GEOMS = {
    'maskfeat': ((3, 7, 7), (2, 4, 4), (1, 3, 3), (2, 4, 32, 32), 448),    # K = 441: 7 pad columns; padding on all six faces
    'tubelet': ((1, 4, 4), (1, 4, 4), (0, 0, 0), (1, 2, 16, 24), 64),      # K = 48: two whole pad groups; no overlap, no padding
    'odd-w': ((3, 3, 3), (1, 2, 2), (1, 1, 1), (1, 3, 10, 23), 88),        # K = 81; 69-byte rows: nothing is 4-byte aligned
}


@pytest.fixture
def norm():
    import vtx
    vtx.set_input_normalization(MEAN, STD)
    yield
    vtx.set_input_normalization(None, None)


def _normalised(u8):
    """ToTensor + Normalize of the reference on a uint8 [B,T,H,W,3] clip -> float [B,T,3,H,W] on the CPU (as
    tests/test_gpu_kernels.py::test_patch_rows_uint8_ingest_bit_exact restates them)."""
    x = u8.permute(0, 1, 4, 2, 3).float().div(255)
    return x.sub(torch.tensor(MEAN).view(1, 1, 3, 1, 1)).div(torch.tensor(STD).view(1, 1, 3, 1, 1)).contiguous()


def _every_byte_clip(shape, seed):
    """Random bytes [B,T,H,W,3] in which every value 0..255 occurs in every channel."""
    u8 = torch.randint(0, 256, tuple(shape) + (3,), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)
    px = u8.view(-1, 3)
    assert px.shape[0] >= 256
    for c in range(3):
        px[37 * c:37 * c + 256, c] = torch.arange(256, dtype=torch.uint8).roll(11 * c)
        assert len(torch.unique(px[:, c])) == 256
    return u8


def _bits(t):
    return t.contiguous().view(BITS[t.dtype])


_gather_refs = {}


def _gather_case(name):
    """Per geometry, computed once: the clip, its normalised float form, pad + unfold of that on the CPU (fp32 rows), and which
    elements of the rows are padding taps."""
    if name not in _gather_refs:
        k3, s3, p3, cs, Kp = GEOMS[name]
        u8 = _every_byte_clip(cs, 3 + len(name))
        xf = _normalised(u8)
        assert bool((xf != 0).all()), 'a normalised value of 0 would hide a padding tap'
        geom = (k3, s3, p3, 3, None, Kp)
        want = P.im2col_ref(xf, geom)
        inside = P.im2col_ref(torch.ones_like(xf), geom) != 0           # False: padding taps and the columns K .. Kp - 1
        _gather_refs[name] = (u8, xf, want, inside)
    return _gather_refs[name]


@pytest.mark.parametrize('dt', ['f32', 'bf16'])
@pytest.mark.parametrize('name', list(GEOMS))
def test_gather_bit_for_bit(name, dt, norm):
    """vtx_im2col3d_u8 on a clip one byte off every alignment, rows NaN on entry with guard rows: equal to vtx_im2col3d of the
    CPU-normalised float clip on the device and to pad + unfold on the CPU (bf16: rounded once), bit pattern for bit pattern;
    padding taps and pad columns are +0.0 (all bits clear) although n(0, c) is not; the guard rows keep their NaN pattern."""
    from vtx import _lib, ops
    k3, s3, p3, (B, T, H, W), Kp = GEOMS[name]
    u8, xf, want, inside = _gather_case(name)
    tdt = TDT[dt]
    M, K = want.shape[0], 3 * k3[0] * k3[1] * k3[2]
    assert want.shape[1] == Kp and Kp % 8 == 0 and Kp >= K
    buf = torch.full((1 + u8.numel() + 64,), 0xA5, dtype=torch.uint8)
    buf[1:1 + u8.numel()] = u8.view(-1)
    buf = buf.to(DEV)
    clip = buf[1:1 + u8.numel()].view(u8.shape)
    assert clip.data_ptr() % 2 == 1 and clip.is_contiguous()
    rows = torch.full((M + TAIL, Kp), float('nan'), dtype=tdt, device=DEV)
    fill = _bits(rows[M:]).cpu().clone()
    mean, std = (ctypes.c_float * 3)(*MEAN), (ctypes.c_float * 3)(*STD)
    _lib.stem_call('vtx_im2col3d_u8', ops._DT[tdt], B, T, H, W, I3(*k3), I3(*s3), I3(*p3), Kp, ops.ptr(clip), mean, std,
                   ops.ptr(rows), ops.stream())
    # the route it replaces, on the device: the float gather of the normalised clip
    ref = torch.full((M, Kp), float('nan'), dtype=tdt, device=DEV)
    xd = xf.to(DEV)
    ops.call('vtx_im2col3d', ops._DT[tdt], B, T, 3, H, W, I3(*k3), I3(*s3), I3(*p3), Kp, ops.ptr(xd), ops.ptr(ref), ops.stream())
    torch.cuda.synchronize()
    got = rows.cpu()
    g, w = _bits(got[:M]), _bits(want.to(tdt))
    bad = (g != w).nonzero()
    assert bad.numel() == 0, f'{name} {dt}: {len(bad)} of {g.numel()} elements differ from pad + unfold, first at {bad[0].tolist()}'
    assert torch.equal(g, _bits(ref.cpu())), f'{name} {dt}: differs from vtx_im2col3d of the normalised float clip'
    assert torch.equal(_bits(got[M:]), fill), f'{name} {dt}: guard rows written'
    assert bool((g[:, K:] == 0).all()), f'{name} {dt}: pad columns are not +0.0'
    assert bool((g[~inside] == 0).all()) and bool((g[inside] != 0).all()), f'{name} {dt}: padding taps are not +0.0'
    if any(p3):
        assert int((~inside[:, :K]).sum()) > 0
    assert bool((buf.cpu()[:1] == 0xA5).all()) and bool((buf.cpu()[1 + u8.numel():] == 0xA5).all())
    # the Python entry gives the same rows
    assert torch.equal(_bits(ops.im2col3d_u8(clip, k3, s3, p3, Kp, tdt).cpu()), g)


def _stem_weights():
    g = torch.Generator().manual_seed(21)
    w = (torch.rand(96, 3, 3, 7, 7, generator=g) - 0.5) * 0.1
    b = torch.rand(96, generator=g) - 0.5
    dy = torch.randn(2, 2 * 8 * 8, 96, generator=g)
    return w, b, dy


@pytest.mark.parametrize('dt', ['f32', 'bf16'])
def test_conv_stem_on_bytes_equals_conv_stem_on_the_normalised_clip(dt, norm):
    """ConvStemFn on the uint8 clip against the same call on the normalised float clip: tokens, d weight and d bias torch.equal."""
    from vtx import functions as F_
    u8, xf, _, _ = _gather_case('maskfeat')
    w0, b0, dy = _stem_weights()
    tdt = TDT[dt]
    res = []
    for clip in (u8.to(DEV), xf.to(DEV)):
        w, b = w0.to(DEV).requires_grad_(True), b0.to(DEV).requires_grad_(True)
        y = F_.ConvStemFn.apply(clip, w, b, (2, 4, 4), (1, 3, 3), tdt)
        y.backward(dy.to(DEV, tdt))
        res.append((y.detach().cpu(), w.grad.cpu(), b.grad.cpu()))
    (y8, w8, b8), (yf, wf, bf) = res
    assert y8.shape == (2, 128, 96) and y8.dtype == tdt and bool(torch.isfinite(y8.float()).all()) and float(y8.float().abs().max()) > 0
    assert torch.equal(y8, yf), f'{dt}: tokens differ'
    assert torch.equal(w8, wf) and float(w8.abs().max()) > 0, f'{dt}: d weight differs'
    assert torch.equal(b8, bf), f'{dt}: d bias differs'


class _StandIn(torch.nn.Module):
    """The small stand-in backbone (as tests/test_gpu_00_baseline_configs.py's): [B, 2*8*8, 96] -> [B, 1 + 2*2*2, 768].  Every
    output token also sees the mean of all pooled tokens: a masked cell's 4x4 input tokens are all the mask token, so without
    that no gradient of the loss would reach the stem and its equality would be one of zeros."""

    def __init__(self):
        super().__init__()
        self.register_buffer('w', torch.randn(768, 96, generator=torch.Generator().manual_seed(4)) * 0.1)

    def forward(self, t):
        t = t.float()
        b = t.shape[0]
        p = t.reshape(b, 2, 2, 4, 2, 4, 96).mean(dim=(3, 5)).reshape(b, 8, 96)
        v = (p + p.mean(1, keepdim=True)) @ self.w.t()
        return torch.cat([v.mean(1, keepdim=True), v], dim=1)


# one masked cell per clip, in different (clip, t') slabs: the mask-token gradient and the loss are then sums of at most two
# atomically added terms each (csrc/hog.hip: mf_blend_bwd_kernel, mf_loss_fwd_kernel), which no arrival order can change --
# equality between two runs is a property of the routes, not of the scheduling
MF_MARKERS = [[[0, 1]], [[1, 1]]]                              # centre frames 1 (t' 0) and 3 (t' 1)


def _mf_mask():
    mask = torch.zeros(2, 2, 2, 2, dtype=torch.int32)
    mask[0, 0, 0, 1] = 1
    mask[1, 1, 1, 0] = 1
    return mask


@pytest.mark.parametrize('prec', ['fp32', 'bf16'])
def test_maskfeat_on_bytes_equals_maskfeat_on_the_normalised_clip(prec, norm):
    """MaskFeat(clip_u8, vtx.hog_targets(clip_u8, markers), ...) against MaskFeat(normalised float clip, the target assembled from
    ops.hog_fwd of the gathered centre frames, ...): pred, loss and the gradients of the stem weight, the mask token and the
    decoder weight are torch.equal, in training mode.  (Without the uint8 stem the first call raises.)"""
    import video_transformer as V
    import vtx
    from vtx import ops
    vtx.set_precision(prec)
    u8, xf, _, _ = _gather_case('maskfeat')
    torch.manual_seed(7)
    m = V.MaskFeat(num_frames=4, img_size=32, pool_q_stride_size=[[1, 1, 2, 2], [3, 1, 2, 2]], feature_dim=2 * 108,
                   backbone=_StandIn()).to(DEV).train()
    mask = _mf_mask().to(DEV)
    clip = u8.to(DEV)
    target_f = torch.zeros(2, 4, 2, 2, 108, dtype=torch.float64, device=DEV)
    for b, c in ((0, 1), (1, 3)):
        target_f[b, c] = ops.hog_fwd(clip[b, c][None].contiguous())[0]
    outs = []
    for route in ('u8', 'float'):
        m.zero_grad()
        if route == 'u8':
            pred, loss = m(clip, vtx.hog_targets(clip, MF_MARKERS), mask, MF_MARKERS)
        else:
            pred, loss = m(xf.to(DEV), target_f, mask, MF_MARKERS)
        loss.backward()
        outs.append([t.detach().cpu().clone() for t in (pred, loss, m.patch_embed.patch_model.weight.grad, m.mask_token.grad,
                                                        m.decoder_pred.weight.grad)])
    a, b = outs
    assert a[0].shape == (2, 4, 2, 2, 108) and a[1].dtype == torch.float64 and float(a[1]) > 0
    for nm, x, y in zip(('pred', 'loss', 'd stem weight', 'd mask_token', 'd decoder_pred weight'), a, b):
        assert bool(torch.isfinite(x).all()), nm
        assert torch.equal(x, y), f'{prec}: {nm} differs between the uint8 and the float route'
    assert float(a[2].abs().max()) > 0 and float(a[3].abs().max()) > 0 and float(a[4].abs().max()) > 0


HOG_MARKERS = [[[0, 1]], [[1, 2], [3, 1]], []]                 # centre frames: clip 0: 1; clip 1: 4 and 7; clip 2: none
HOG_CENTRES = [(0, 1), (1, 4), (1, 7)]


def test_hog_targets(norm):
    """B=3, T=8, 32x48: the target equals zeros with hog_fwd(clip[b, centre]) scattered in, bit for bit; every frame equals the
    CPU oracle (extract_hog_features), and so does vtx_hog_fwd on the same frames (unchanged); every other row is exactly zero;
    a duplicated marker changes nothing; a centre of T raises ValueError."""
    import vtx
    from oracle import hog_oracle as H
    from vtx import ops
    u8 = torch.randint(0, 256, (3, 8, 32, 48, 3), generator=torch.Generator().manual_seed(17), dtype=torch.uint8)
    clip = u8.to(DEV)
    got = vtx.hog_targets(clip, HOG_MARKERS)
    assert got.shape == (3, 8, 2, 3, 108) and got.dtype == torch.float64 and got.device == clip.device
    frames = torch.stack([clip[b, c] for b, c in HOG_CENTRES]).contiguous()
    dense = ops.hog_fwd(frames)
    want = torch.zeros_like(got)
    for i, (b, c) in enumerate(HOG_CENTRES):
        want[b, c] = dense[i]
    g, w = got.cpu(), want.cpu()
    assert torch.equal(g.view(torch.int64), w.view(torch.int64)), 'hog_targets differs from hog_fwd of the gathered frames'
    keep = torch.zeros(3, 8, dtype=torch.bool)
    for b, c in HOG_CENTRES:
        keep[b, c] = True
        oracle = H.extract_hog_features(u8[b, c].numpy())
        assert np.array_equal(g[b, c].numpy(), oracle), f'hog_targets of clip {b} frame {c} differs from the oracle'
        assert np.array_equal(dense[HOG_CENTRES.index((b, c))].cpu().numpy(), oracle), 'vtx_hog_fwd differs from the oracle'
        assert float(g[b, c].abs().max()) > 0
    assert bool((g[~keep].view(torch.int64) == 0).all()), 'a row that was not selected is not +0.0'
    assert bool((g[2] == 0).all())
    twice = vtx.hog_targets(clip, [[[0, 1], [0, 1]], [[3, 1], [1, 2], [3, 1]], []])
    assert torch.equal(twice.cpu().view(torch.int64), g.view(torch.int64))
    assert bool((vtx.hog_targets(clip, [[], [], []]) == 0).all())
    with pytest.raises(ValueError, match='centre frame'):
        vtx.hog_targets(clip, [[[3, 2]], [], []])              # 3*2 + 2*2//2 = 8 = T
    with pytest.raises(ValueError, match='multiples of 16'):
        vtx.hog_targets(clip[:, :, :24], HOG_MARKERS)
    with pytest.raises(ValueError, match='marker lists'):
        vtx.hog_targets(clip, HOG_MARKERS[:2])


def test_errors():
    """uint8 without set_input_normalization: ValueError (patch_rows' message); a [B,T,3,H,W] uint8 tensor: ValueError; a
    MixedClip: the TypeError of before."""
    import mvit
    import video_transformer as V
    import vtx
    from vtx import functions as F_, ops
    clip = torch.zeros(2, 4, 32, 32, 3, dtype=torch.uint8, device=DEV)
    stem = mvit.create_conv_patch_embed(in_channels=3, out_channels=96, conv_kernel_size=(3, 7, 7), conv_stride=(2, 4, 4),
                                        conv_padding=(1, 3, 3)).to(DEV)
    mf = V.MaskFeat(num_frames=4, img_size=32, pool_q_stride_size=[[1, 1, 2, 2], [3, 1, 2, 2]], feature_dim=216,
                    backbone=_StandIn()).to(DEV)
    vtx.set_input_normalization(None, None)
    for call in (lambda: ops.im2col3d_u8(clip, (3, 7, 7), (2, 4, 4), (1, 3, 3), 448, F32), lambda: stem(clip),
                 lambda: mf.forward_features(clip)):
        with pytest.raises(ValueError, match='set_input_normalization'):
            call()
    vtx.set_input_normalization(MEAN, STD)
    try:
        planar = clip.permute(0, 1, 4, 2, 3).contiguous()      # [B,T,3,H,W] uint8
        pm = stem.patch_model
        for call in (lambda: ops.im2col3d_u8(planar, (3, 7, 7), (2, 4, 4), (1, 3, 3), 448, F32), lambda: stem(planar),
                     lambda: mf.forward_features(planar), lambda: vtx.hog_targets(planar, [[], []]),
                     lambda: F_.ConvStemFn.apply(planar, pm.weight, pm.bias, (2, 4, 4), (1, 3, 3), F32)):
            with pytest.raises(ValueError, match=r'\[B,T,H,W,3\]'):
                call()
        carrier = vtx.MixedClip(clip, 0.3)
        with pytest.raises(TypeError, match='MixedClip'):
            stem(carrier)
        with pytest.raises(TypeError, match='MixedClip'):
            mf.forward_features(carrier)
        assert stem(clip).shape == (2, 128, 96)                # and the clip itself goes through
    finally:
        vtx.set_input_normalization(None, None)
