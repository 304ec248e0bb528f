"""Test-time views on the device (csrc/views.hip, vtx.ops.clip_views_u8, vtx.aug.ClipTest and ``frames=``): byte identity with
the existing resampler on the gathered frames, the float64 evaluation of the tables, guard bytes, table overrun, the classes,
the path into a model and the trainer's test_step."""
import types

import numpy as np
import pytest
import torch

import aug_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SEED = 11

#: name -> (clips, decoded frames, source (Hs, Ws), y spec, x spec, rows (first, one past last), lefts, width, frames).  A spec is
#: (crop start, crop length, output length, flip) of one axis; every clip of a case shares it.
CASES = {
    # 40x56 -> 36x50 (ClipTest(32, short_side=36)'s geometry): every view holds columns no other holds, frames repeat
    'three-crop': (2, 5, (40, 56), (0, 40, 36, False), (0, 56, 50, False), (2, 34), [0, 18, 9], 32, [[0, 2, 4], [1, 1, 3]]),
    # 56x40 -> 50x36: lefts 0, 4, 2 -- columns 4 .. 31 lie in all three views
    'tall': (2, 5, (56, 40), (0, 56, 50, False), (0, 40, 36, False), (9, 41), [0, 4, 2], 32, [[0, 2, 4], [1, 1, 3]]),
    # 40x57 -> 33x47, 29 rows: the last band of eight rows holds five; row and window lengths that are odd
    'odd': (2, 3, (40, 57), (0, 40, 33, False), (0, 57, 47, False), (2, 31), [0, 18, 9], 29, [[2, 0], [1, 1]]),
    # the wide case of tests/test_gpu_aug.py: box (1, 2, 10, 297) of 12x301 -> 10x270, flipped: two column tiles, views that
    # do not touch, and columns 10 .. 129, 140 .. 259 in no view
    'wide': (1, 3, (12, 301), (1, 10, 10, False), (2, 297, 270, True), (0, 10), [0, 260, 130], 10, [[2, 0, 1]]),
}
FLOAT64_CASES = ('three-crop', 'tall', 'odd')


def _stack_tables(B, src_len, spec, rows, mode, antialias, spare=True):
    """One table per clip, cut to ``rows`` -> (host table, stacked device triple).  spare: one more weight column than the
    widest window, NaN behind every count -- a kernel that read past a count would show it."""
    from vtx import ops
    start, length, out_len, flip = spec
    taps = ops.resample_max_taps(length, out_len, mode, antialias) + (1 if spare else 0)
    f, c, w = ops.resample_table(src_len, start, length, out_len, mode, antialias, flip=flip, max_taps=taps)
    if spare:
        for o in range(len(f)):
            w[o, c[o]:] = np.nan
        assert np.isnan(w).any(axis=1).all()
    host = tuple(a[rows[0]:rows[1]] for a in (f, c, w))
    dev = tuple(torch.from_numpy(np.stack([a] * B)).to(DEV) for a in host)
    return host, dev


def _case(name, mode, antialias, spare=True):
    B, Ts, (Hs, Ws), yspec, xspec, rows, lefts, width, frames = CASES[name]
    src = R.source_clip(B, Ts, (Hs, Ws), seed=SEED)
    yhost, ydev = _stack_tables(B, Hs, yspec, rows, mode, antialias, spare)
    xhost, xdev = _stack_tables(B, Ws, xspec, (0, xspec[2]), mode, antialias, spare)
    return types.SimpleNamespace(B=B, Ts=Ts, src=src, frames=frames, lefts=[lefts] * B, width=width, H=rows[1] - rows[0], Wr=xspec[2],
                                 yhost=yhost, ydev=ydev, xhost=xhost, xdev=xdev)


def _gathered(c):
    return torch.stack([c.src[b, c.frames[b]] for b in range(c.B)])


def _sliced(whole, c):
    """[B,T,H,Wr,3] -> [B,V,T,H,W,3]: the windows of the whole resized rows."""
    return torch.stack([torch.stack([whole[b, :, :, l:l + c.width] for l in c.lefts[b]]) for b in range(c.B)])


@pytest.mark.parametrize('mode,antialias', R.MODES)
@pytest.mark.parametrize('name', list(CASES))
def test_views_equal_the_resampler_on_the_gathered_frames(name, mode, antialias):
    """Byte identity with vtx_clip_resample_u8 (same tables, NaN behind every tap count) on src[b, frames[b]], sliced per view;
    for the first three cases also the float64 rule of tests/test_gpu_aug.py: exact except +-1 within R.TIE of a rounding tie."""
    from vtx import ops
    c = _case(name, mode, antialias)
    got = ops.clip_views_u8(c.src.to(DEV), c.frames, c.lefts, c.width, c.xdev, c.ydev)
    whole = ops.clip_resample_u8(_gathered(c).to(DEV), (c.H, c.Wr), c.xdev, c.ydev)
    torch.cuda.synchronize()
    T = len(c.frames[0])
    assert got.shape == (c.B, 3, T, c.H, c.width, 3) and got.dtype == torch.uint8 and got.is_contiguous()
    got, want = got.cpu(), _sliced(whole.cpu(), c)
    assert torch.equal(got, want), f'{int((got != want).sum())} bytes differ'
    if name in FLOAT64_CASES:
        v64 = np.stack([R.table_eval(c.src[b, c.frames[b]].numpy(), c.yhost, c.xhost) for b in range(c.B)])
        v64 = _sliced(torch.from_numpy(v64), c).numpy()
        tie = R.near_tie(v64)
        diff = np.abs(got.numpy().astype(np.float64) - np.rint(np.clip(v64, 0.0, 255.0)))
        print(f'{name} {mode} antialias={antialias}: tie share {tie.mean():.4f}, bytes off {int((diff > 0).sum())}, max diff {diff.max():.0f}')
        assert tie.mean() <= R.TIE_SHARE
        assert np.all((diff == 0) | (tie & (diff <= 1)))
    if name == 'three-crop':
        assert np.all(got[0, :, 0].numpy() == 0) and np.any(got[0, :, 1].numpy() != 0)        # frame 0 of clip 0 is all 0
    # device index tensors are taken as they are
    dev_i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)
    again = ops.clip_views_u8(c.src.to(DEV), dev_i32(c.frames), dev_i32(c.lefts), c.width, c.xdev, c.ydev)
    assert torch.equal(again.cpu(), got)


def test_views_edges_of_the_band_byte_for_byte():
    """40x300 -> 13 rows x 772 columns (bicubic, antialias: y windows of up to 15 taps), views of 60 columns from 0, 30 and 712,
    tables bent per clip (aug_ref.edge_table): columns 30 .. 59 lie in two views, the column tile 256 .. 511 in none, the last
    tile has 4 live lanes, the last band 5 rows; windows past the source edge, counts above the taps and of 0.  Against the
    float32 restatement of the kernel (aug_ref.resample_f32) on the gathered frames, sliced: every byte equal."""
    from vtx import ops
    B, Ts, (Hs, Ws), (H, Wr), W = 2, 3, (40, 300), (13, 772), 60
    frames, lefts = [[1, 0], [0, 2]], [[0, 30, 712]] * B
    src = R.source_clip(B, Ts, (Hs, Ws), seed=SEED)
    ytabs, xtabs = [R.edge_table(Hs, H, shift=b) for b in range(B)], [R.edge_table(Ws, Wr, shift=b) for b in range(B)]
    assert max(int(R.kernel_windows(t, Hs)[1].max()) for t in ytabs) > 8
    dev = lambda tabs: tuple(torch.from_numpy(np.stack([t[i] for t in tabs])).to(DEV) for i in range(3))
    got = ops.clip_views_u8(src.to(DEV), frames, lefts, W, dev(xtabs), dev(ytabs))
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    whole = [R.resample_f32(src[b, frames[b]].numpy(), ytabs[b], xtabs[b]) for b in range(B)]
    want = np.stack([np.stack([whole[b][:, :, l:l + W] for l in lefts[b]]) for b in range(B)])
    assert got.shape == (B, 3, 2, H, W, 3) and np.array_equal(got, want), f'{int((got != want).sum())} bytes differ'
    assert np.array_equal(got[:, 0, :, :, 30:], got[:, 1, :, :, :30])                      # the columns that two views hold
    for b in range(B):
        assert not got[b, :, :, 6 + b].any() and not got[b, 0, :, :, 6 + b].any() and got[b, 2, 0, 5].any()


@pytest.mark.parametrize('mode,antialias', R.MODES)
def test_one_view_of_every_frame_is_the_plain_call(mode, antialias):
    """V = 1, frames=None, the window = the whole row: vtx_clip_resample_u8 itself."""
    from vtx import ops
    c = _case('three-crop', mode, antialias)
    got = ops.clip_views_u8(c.src.to(DEV), None, [[0]] * c.B, c.Wr, c.xdev, c.ydev)
    want = ops.clip_resample_u8(c.src.to(DEV), (c.H, c.Wr), c.xdev, c.ydev)
    assert got.shape == (c.B, 1, c.Ts, c.H, c.Wr, 3)
    assert torch.equal(got[:, 0], want)


def test_out_argument_leaves_every_byte_around_it():
    from vtx import ops
    c = _case('odd', 'bicubic', False)
    shape = (c.B, 3, len(c.frames[0]), c.H, c.width, 3)
    n, pad = int(np.prod(shape)), 4099
    buf = torch.full((pad + n + pad,), 0xA5, dtype=torch.uint8, device=DEV)
    out = buf[pad:pad + n].view(shape)
    ret = ops.clip_views_u8(c.src.to(DEV), c.frames, c.lefts, c.width, c.xdev, c.ydev, out=out)
    want = ops.clip_views_u8(c.src.to(DEV), c.frames, c.lefts, c.width, c.xdev, c.ydev)
    torch.cuda.synchronize()
    assert ret.data_ptr() == out.data_ptr()
    assert bool((buf[:pad] == 0xA5).all()) and bool((buf[pad + n:] == 0xA5).all())
    assert torch.equal(out, want) and bool((want != 0xA5).any())


@pytest.mark.parametrize('mode,antialias', [('bilinear', False), ('bicubic', True)])
def test_weights_behind_a_tap_count_are_never_read(mode, antialias):
    """One spare NaN weight column behind the widest window against tables without it: the same bytes."""
    from vtx import ops
    c, d = _case('three-crop', mode, antialias, spare=True), _case('three-crop', mode, antialias, spare=False)
    assert bool(torch.isnan(c.xdev[2]).any()) and bool(torch.isnan(c.ydev[2]).any()) and c.xdev[2].shape[2] == d.xdev[2].shape[2] + 1
    assert not bool(torch.isnan(d.xdev[2]).any())
    a = ops.clip_views_u8(c.src.to(DEV), c.frames, c.lefts, c.width, c.xdev, c.ydev)
    b = ops.clip_views_u8(d.src.to(DEV), d.frames, d.lefts, d.width, d.xdev, d.ydev)
    assert torch.equal(a, b)


@pytest.mark.parametrize('mode,antialias', [('bilinear', False), ('bicubic', True)])
def test_clip_test_is_resize_then_three_crop(mode, antialias):
    """ClipTest(32, short_side=36) on 40x56: the whole frame resized to 36x50, then rows 2 .. 34 and columns from 0, 18, 9; view v
    of clip b in row b * 3 + v; with frames= the same of the gathered clip."""
    from vtx import aug, ops
    clip = R.source_clip(2, 5, R.SRC_HW, seed=SEED)
    t = aug.ClipTest(32, short_side=36, interpolation=mode, antialias=antialias)
    up = lambda tab: tuple(torch.from_numpy(np.stack([a] * 2)).to(DEV) for a in tab)
    ytab, xtab = up(ops.resample_table(40, 0, 40, 36, mode, antialias)), up(ops.resample_table(56, 0, 56, 50, mode, antialias))
    frames = [[0, 2, 4], [1, 1, 3]]
    for fr, src in ((None, clip), (frames, torch.stack([clip[b, frames[b]] for b in range(2)]))):
        got = t(clip.to(DEV), frames=fr)
        whole = ops.clip_resample_u8(src.to(DEV), (36, 50), xtab, ytab)
        assert got.shape == (6, src.shape[1], 32, 32, 3) and got.dtype == torch.uint8 and got.is_cuda
        for b in range(2):
            for v, left in enumerate((0, 18, 9)):
                assert torch.equal(got[b * 3 + v], whole[b, :, 2:34, left:left + 32]), (b, v)
    assert torch.equal(t(clip.to(DEV), frames=[4, 0]), t(clip.to(DEV), frames=[[4, 0], [4, 0]]))      # [T]: every clip alike


@pytest.mark.parametrize('auto_augment', [None, 'rand-m9-mstd0.5-inc1'])
def test_frames_argument_equals_the_call_on_the_gathered_clip(auto_augment):
    """ClipEval and ClipAugment (colour jitter, and RandAugment) with frames= against frames=None on clips[b, frames[b]], same draws."""
    from vtx import aug
    clip = R.source_clip(2, 5, R.SRC_HW, seed=SEED)
    frames = [[0, 2, 4], [1, 1, 3]]
    gathered = torch.stack([clip[b, frames[b]] for b in range(2)]).to(DEV)
    e = aug.ClipEval(img_size=32)
    got = e(clip.to(DEV), frames=frames)
    assert got.shape == (2, 3, 32, 32, 3) and torch.equal(got, e(gathered))
    a = aug.ClipAugment(img_size=32, auto_augment=auto_augment)
    draws = aug.sample_params(2, R.SRC_HW, generator=torch.Generator().manual_seed(9), auto_augment=auto_augment, out_hw=(32, 32))
    assert all(len(d.randaug) == 2 for d in draws) if auto_augment else all(len(d.ops) == 3 for d in draws)
    got = a(clip.to(DEV), params=draws, frames=np.array(frames))
    assert got.shape == (2, 3, 32, 32, 3) and torch.equal(got, a(gathered, params=draws))
    assert torch.equal(got, a(clip.to(DEV), generator=torch.Generator().manual_seed(9), frames=torch.tensor(frames)))


def test_clip_test_feeds_the_models():
    """ClipTest's uint8 views under set_input_normalization through a one-layer TimeSformer = the model on the float clip
    (views / 255 - mean) / std."""
    import vtx
    import video_transformer as V
    from model_common import _build
    from vtx import aug
    clip = R.source_clip(2, 5, R.SRC_HW, seed=SEED)
    out = aug.ClipTest(32, short_side=36)(clip.to(DEV), frames=[[0, 2, 4], [1, 1, 3]])
    assert out.shape == (6, 3, 32, 32, 3)
    mean, std = [0.45, 0.45, 0.45], [0.225, 0.225, 0.225]
    xf = out.cpu().permute(0, 1, 4, 2, 3).float().div(255)
    xf = xf.sub(torch.tensor(mean).view(1, 1, 3, 1, 1)).div(torch.tensor(std).view(1, 1, 3, 1, 1))
    vtx.set_precision('fp32')
    try:
        m, _ = _build(V.TimeSformer, 5, num_frames=3, img_size=32, patch_size=16, embed_dims=128, num_heads=2, num_transformer_layers=1)
        m.eval()
        vtx.set_input_normalization(mean, std)
        with torch.no_grad():
            y8 = m(out)
            yf = m(xf.to(DEV))
    finally:
        vtx.set_input_normalization(None, None)
        vtx.set_precision('auto')
    assert y8.shape[0] == 6 and torch.equal(y8, yf)


def test_test_step_takes_the_stacked_views():
    """test_step on [B, n_crops, T, C, H, W] = test_step on the flattened [B * n_crops, T, C, H, W]: the same logits, one
    prediction per clip."""
    import vtx
    import model_trainer as MT
    cfg = types.SimpleNamespace(objective='supervised', arch='timesformer', pretrain_pth=None, weights_from='imagenet', img_size=32,
                                num_frames=2, attention_type='divided_space_time', num_class=10, eval_metrics='finetune', mixup=False,
                                optim_type='sgd', lr=0.05, weight_decay=0.05, weight_decay_end=0.01, lr_schedule='cosine', warmup_epochs=2,
                                min_lr=1e-4, clip_grad=0.5, layer_decay=1, save_ckpt_freq=1)
    vtx.set_precision('fp32')
    try:
        torch.manual_seed(0)
        trainer = types.SimpleNamespace(max_epochs=10, current_epoch=3, save_checkpoint=lambda p: None)
        m = MT.VideoTransformer(cfg, trainer, ckpt_dir='.', do_eval=False, do_test=True)
        m.to(DEV).eval()
        logits = []
        m.cls_head.register_forward_hook(lambda mod, args, out: logits.append(out.detach().clone()))
        g = torch.Generator().manual_seed(1)
        x = torch.randn(2, 3, 2, 3, 32, 32, generator=g).to(DEV)
        y = torch.randint(0, 10, (2,), generator=g).to(DEV)
        with torch.no_grad():
            m.test_step((x, y), 0)
            six = (m.test_top1_acc.correct.clone(), m.test_top1_acc.total, m.test_top5_acc.correct.clone())
            m.test_top1_acc.reset()
            m.test_top5_acc.reset()
            m.test_step((x.reshape(6, 2, 3, 32, 32), y), 1)
        torch.cuda.synchronize()
    finally:
        vtx.set_precision('auto')
    assert len(logits) == 2 and logits[0].shape == (6, 10) and torch.equal(logits[0], logits[1])
    assert six[1] == m.test_top1_acc.total == 2
    assert torch.equal(six[0], m.test_top1_acc.correct) and torch.equal(six[2], m.test_top5_acc.correct)


def test_bad_arguments_raise_and_launch_nothing():
    from vtx import aug, ops
    c = _case('three-crop', 'bilinear', False)
    src = c.src.to(DEV)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)
    ops.profile_start(('clip_views',))
    try:
        for frames in ([[0, 2, 5], [1, 1, 3]], [[0, 2, 4], [-1, 1, 3]]):                           # frame index out of range
            with pytest.raises(ValueError, match='frame'):
                ops.clip_views_u8(src, frames, c.lefts, c.width, c.xdev, c.ydev)
            with pytest.raises(ValueError, match='outside the 5 decoded frames'):
                aug.ClipTest(32, short_side=36)(src, frames=frames)
            with pytest.raises(ValueError, match='outside the 5 decoded frames'):
                aug.ClipEval(32)(src, frames=frames)
            with pytest.raises(ValueError, match='outside the 5 decoded frames'):
                aug.ClipAugment(32)(src, frames=frames)
        for lefts in ([[0, 19, 9]] * 2, [[-1, 18, 9]] * 2):                                        # left + width > Wr
            with pytest.raises(ValueError, match='left'):
                ops.clip_views_u8(src, c.frames, lefts, c.width, c.xdev, c.ydev)
        with pytest.raises(ValueError, match='do not fit'):
            ops.clip_views_u8(src, c.frames, [[0]] * 2, 51, c.xdev, c.ydev)
        for lefts in ([[0] * 9] * 2, i32([[0] * 9] * 2)):                                          # V > 8
            with pytest.raises(ValueError, match='at most 8'):
                ops.clip_views_u8(src, c.frames, lefts, c.width, c.xdev, c.ydev)
        with pytest.raises(TypeError):                                                             # wrong dtypes and shapes
            ops.clip_views_u8(src.float(), c.frames, c.lefts, c.width, c.xdev, c.ydev)
        with pytest.raises(TypeError):
            ops.clip_views_u8(src, [[0.0, 2.0, 4.0]] * 2, c.lefts, c.width, c.xdev, c.ydev)
        with pytest.raises(TypeError):
            ops.clip_views_u8(src, i32(c.frames).long(), c.lefts, c.width, c.xdev, c.ydev)
        with pytest.raises(TypeError):
            ops.clip_views_u8(src, c.frames, i32(c.lefts).float(), c.width, c.xdev, c.ydev)
        with pytest.raises(TypeError):
            ops.clip_views_u8(src, c.frames, [[0, 18, 9]], c.width, c.xdev, c.ydev)                # one row for two clips
        with pytest.raises(TypeError):
            ops.clip_views_u8(src, c.frames, c.lefts, c.width, (c.xdev[0], c.xdev[1], c.xdev[2].double()), c.ydev)
        with pytest.raises(TypeError):
            ops.clip_views_u8(src, c.frames, c.lefts, c.width, c.xdev, (c.ydev[0][:1], c.ydev[1], c.ydev[2]))
        with pytest.raises(TypeError):
            ops.clip_views_u8(src, c.frames, c.lefts, c.width, c.xdev, c.ydev, out=torch.empty(2, 3, 3, 32, 32, 3, device=DEV))
        with pytest.raises(TypeError):
            ops.clip_views_u8(src, c.frames, c.lefts, c.width, c.xdev, c.ydev, out=torch.empty(2, 3, 3, 32, 31, 3, dtype=torch.uint8, device=DEV))
        with pytest.raises(TypeError, match='host integers'):
            aug.ClipTest(32, short_side=36)(src, frames=i32(c.frames))
        with pytest.raises(ValueError, match='bigger than input size'):
            aug.ClipTest(40, short_side=36)(src)
        torch.cuda.synchronize()
    finally:
        launched = ops.profile_stop()
    assert launched == {'clip_views': {}}
