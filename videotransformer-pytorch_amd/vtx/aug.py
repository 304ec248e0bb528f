"""Clip augmentation on the device: the transforms of the reference's ``transforms_train`` / ``transforms_eval``
(data_transform.py:495-574) and of its test pipeline (data_trainer.py:108-121) that run before ToTensor + Normalize, on decoded
uint8 clips [B,T,H,W,3].

    aug = vtx.aug.ClipAugment(img_size=224)             # RandomResizedCrop (bicubic) + flip + ColorJitter(0.4, 0.4, 0.4)
    aug = vtx.aug.ClipAugment(img_size=224, auto_augment='rand-m9-mstd0.5-inc1')      # ... + RandAugment() instead of the jitter
    vtx.set_input_normalization(mean, std)              # ToTensor + Normalize: fused into the patch gather
    out = model(aug(clip_u8.cuda()))

    mixup_fn = mixup.Mixup(num_classes=num_class)       # the -mixup flag (model_trainer.py:87-88,142-143), on the same uint8 clips:
    inputs, soft = mixup_fn(aug(clip_u8.cuda()), labels)  # CutMix swaps the box of bytes in place; Mixup returns a vtx.MixedClip,
    out = model(inputs)                                 # which the patch gather normalises and mixes on the fly (libvtx_mix.so)

    idx = vtx.aug.sample_frames(len(video), num_frames=8, frame_interval=32)           # TemporalRandomCrop + np.linspace
    views = vtx.aug.ClipTest(img_size=224)(decoded_u8.cuda(), frames=[idx])             # Resize(256) + ThreeCrop: [B*3,T,224,224,3]
    preds = head(model(views)).view(-1, 3, num_class).mean(1)

    aug = vtx.aug.ClipAugment(img_size=224, scale=(0.5, 1.0), color_jitter=None)       # the mim branch (data_trainer.py:61-63)
    clip = aug(clip_u8.cuda())                          # uint8 [B,16,224,224,3]
    target = vtx.hog_targets(clip, cube_marker)         # HOG of each masked cube's centre frame (dataset.py:188-196), zeros elsewhere
    pred, loss = maskfeat(clip, target, mask, cube_marker)   # the MViT stem gathers and normalises the bytes (libvtx_stem.so)

What is random is drawn on the host (``sample_params``: torchvision's draws restated, under a ``torch.Generator``), once per
clip -- every frame of a clip gets the same crop, flip and colour factors, as the reference's single call on a [T,C,H,W]
tensor does.  The pixels are touched by libvtx_aug.so (csrc/aug.hip, include/vtx_aug.h): ``vtx_clip_resample_u8`` and
``vtx_clip_jitter_u8``, and, under ``auto_augment``, by libvtx_randaug.so (csrc/randaug.hip, include/vtx_randaug.h).  Every
pipeline takes ``frames=``, indices into the decoded frames (``sample_frames``); with it, and in ``ClipTest`` always, the
resampling is libvtx_views.so's (csrc/views.hip, include/vtx_views.h): frame gather, resize and all crops in one launch.

``auto_augment``: as in the reference (data_transform.py:520-521) any truthy value selects ``RandAugment()`` with its defaults
(two ops of fourteen at magnitude bin 9 of 31, nearest interpolation, no fill) and the content of the string is ignored.  What
is restated is torchvision's tensor path as of 0.13 .. 0.20; torchvision is not a dependency and no version is pinned.

Clips that differ in size: every pipeline also takes a list (or tuple) of B clips [Ts_b,Hs_b,Ws_b,3], each its own tensor with its
own decoded length and frame size -- what a loader yields that collates decoded videos as they are -- and returns the same
uniform [B,T,S,S,3] ([B*3,T,S,S,3] for ``ClipTest``) in the same number of launches: the resampling is then libvtx_ragged.so's
(csrc/ragged.hip, include/vtx_ragged.h), which reads each clip's base pointer and geometry on the device.

    batch = [c.cuda(non_blocking=True) for c in decoded]          # 340x256, 256x340, 320x240, ...: no resize on the host
    out = model(aug(batch, frames=[vtx.aug.sample_frames(len(c), 8, 4) for c in decoded]))

Decoded 4:2:0 frames: no decoder yields RGB -- ffmpeg-based readers get [T,H,W,3] by a colour conversion on the CPU workers
(dataset.py:101-113,163), the GPU's decode engines write NV12 -- so every pipeline also takes a list (or tuple) of ``vtx.YUVClip``,
NV12 or I420 planes as the decoder left them, of their own sizes, pitches and matrices, wherever it takes a list of uint8 clips:
half the bytes over PCIe and into the resampler, which converts each tap in registers (libvtx_yuv.so: csrc/yuv.hip,
include/vtx_yuv.h) and returns the same uniform uint8 RGB result, byte for byte that of the converted clips
(``ops.yuv420_to_rgb_u8``).  A list holds tensors or YUVClip, not both.

    batch = [vtx.YUVClip(y.cuda(non_blocking=True), uv.cuda(non_blocking=True)) for y, uv in decoded_nv12]      # matrix='bt601'
    out = model(aug(batch, frames=[vtx.aug.sample_frames(len(c), 8, 4) for c in batch]))

10-bit streams (HEVC Main10, AV1; P010 from the decode engines, yuv420p10le from ffmpeg-based readers) are int16 / uint16 planes
of the same shapes, ``vtx.YUVClip(y, uv, depth=10)``, and go into the same list beside 8-bit clips: a list with a 10-bit clip in
it is one launch of libvtx_yuv10.so (csrc/yuv10.hip, include/vtx_yuv10.h) for all of its clips.

Not built: RandomGrayscale, hue jitter, RandAugment's ``fill`` and other interpolations.
"""
import math
from collections import namedtuple

import numpy as np
import torch

from . import ops

#: one clip's draws: crop box (rows top .. top+height, columns left .. left+width of the source frame), the flip coin and the
#: colour ops in the order they are applied (0 brightness, 1 contrast, 2 saturation) with their factors; ``randaug``: the
#: (op index, signed magnitude) pairs of RandAugment in the order they are applied (``sample_randaug``), () without auto_augment
ClipDraw = namedtuple('ClipDraw', 'top left height width flip ops factors randaug', defaults=[()])

#: torchvision's RandAugment._augmentation_space, in its order (the op index is the position)
RANDAUG_OPS = ('Identity', 'ShearX', 'ShearY', 'TranslateX', 'TranslateY', 'Rotate', 'Brightness', 'Color', 'Contrast', 'Sharpness',
               'Posterize', 'Solarize', 'AutoContrast', 'Equalize')
_RA_SIGNED = frozenset(range(1, 10))
_RA_JITTER = {6: 0, 7: 2, 8: 1}          # Brightness, Color, Contrast -> op of vtx_clip_jitter_u8 (0 brightness, 2 saturation, 1 contrast)


def sample_frames(total_frames, num_frames, frame_interval, generator=None):
    """The frame indices the reference's datasets read of a video of ``total_frames`` decoded frames (dataset.py:160-162):
    ``TemporalRandomCrop(num_frames * frame_interval)`` (data_transform.py:475-489) -- a window of that many frames that begins
    uniformly on 0 .. max(0, total - size - 1) and is cut at the end of the video -- then
    ``np.linspace(begin, end - 1, num_frames, dtype=int)``.  The draw comes from ``generator`` (None = torch's default CPU
    generator), not from Python's ``random``.  -> int64 array [num_frames].  ValueError where the reference's
    ``assert end - begin >= num_frames`` fires (it then draws another video)."""
    total, n = int(total_frames), int(num_frames)
    size = n * int(frame_interval)
    if n < 1 or size < n or total < 1:
        raise ValueError(f'sample_frames: num_frames={num_frames}, frame_interval={frame_interval}, total_frames={total_frames} must be positive')
    rand_end = max(0, total - size - 1)
    begin = int(torch.randint(0, rand_end + 1, (1,), generator=generator))
    end = min(begin + size, total)
    if end - begin < n:
        raise ValueError(f'sample_frames: a video of {total} frames is shorter than the {n} frames asked for')
    return np.linspace(begin, end - 1, n, dtype=int)


def _check_frames(frames, B, Ts):
    """frames= of the pipelines: host integers [B,T], or [T] for every clip alike, indices into the Ts decoded frames -> int32 [B,T]."""
    if isinstance(frames, torch.Tensor):
        if frames.is_cuda:
            raise TypeError('frames: host integers expected (a list, an array or a CPU tensor), got a device tensor')
        frames = frames.numpy()
    a = np.asarray(frames)
    if a.dtype.kind not in 'iu' or a.ndim not in (1, 2) or a.size == 0:
        raise TypeError(f'frames: integers [T] or [{B},T] expected, got {a.dtype} {a.shape}')
    if a.ndim == 1:
        a = np.broadcast_to(a, (B, a.shape[0]))
    if a.shape[0] != B:
        raise ValueError(f'frames: {a.shape[0]} rows for {B} clips')
    if a.min() < 0 or a.max() >= Ts:
        raise ValueError(f'frames: indices {int(a.min())} .. {int(a.max())} outside the {Ts} decoded frames')
    return np.ascontiguousarray(a, dtype=np.int32)


def _check_frames_ragged(frames, lengths):
    """frames= for a list of clips of ``lengths`` decoded frames: B rows of T host integers, row b indices into its own clip's
    frames, or one row [T] for every clip -> int32 [B,T]; None (every frame) needs clips of one length."""
    B = len(lengths)
    if frames is None:
        if len(set(lengths)) != 1:
            raise ValueError(f'frames: clips of {list(lengths)} decoded frames: without frames= every frame is taken and the lengths must agree')
        return None
    if isinstance(frames, torch.Tensor):
        if frames.is_cuda:
            raise TypeError('frames: host integers expected (a list, an array or a CPU tensor), got a device tensor')
        frames = frames.numpy()
    try:
        a = np.asarray(frames)
    except ValueError as e:                                      # rows of different lengths
        raise TypeError(f'frames: integers [T] or [{B},T] expected: {e}') from e
    if a.dtype.kind not in 'iu' or a.ndim not in (1, 2) or a.size == 0:
        raise TypeError(f'frames: integers [T] or [{B},T] expected, got {a.dtype} {a.shape}')
    if a.ndim == 1:
        a = np.broadcast_to(a, (B, a.shape[0]))
    if a.shape[0] != B:
        raise ValueError(f'frames: {a.shape[0]} rows for {B} clips')
    bad = ((a < 0) | (a >= np.asarray(lengths).reshape(B, 1))).any(axis=1)
    if bad.any():
        b = int(np.argmax(bad))
        raise ValueError(f'frames: indices {int(a[b].min())} .. {int(a[b].max())} of clip {b} outside its {lengths[b]} decoded frames')
    return np.ascontiguousarray(a, dtype=np.int32)


def _uniform(lo, hi, generator):
    return float(torch.empty(1).uniform_(float(lo), float(hi), generator=generator))


def _crop_box(height, width, scale, ratio, generator):
    """torchvision RandomResizedCrop.get_params: ten tries of (uniform area, log-uniform ratio), then the centre crop with the
    ratio clamped into range."""
    area = height * width
    log_ratio = torch.log(torch.tensor([float(ratio[0]), float(ratio[1])]))
    for _ in range(10):
        target_area = area * _uniform(scale[0], scale[1], generator)
        aspect = float(torch.exp(torch.empty(1).uniform_(float(log_ratio[0]), float(log_ratio[1]), generator=generator)))
        w = int(round(math.sqrt(target_area * aspect)))
        h = int(round(math.sqrt(target_area / aspect)))
        if 0 < w <= width and 0 < h <= height:
            top = int(torch.randint(0, height - h + 1, size=(1,), generator=generator))
            left = int(torch.randint(0, width - w + 1, size=(1,), generator=generator))
            return top, left, h, w
    in_ratio = float(width) / float(height)
    if in_ratio < min(ratio):
        w = width
        h = int(round(w / min(ratio)))
    elif in_ratio > max(ratio):
        h = height
        w = int(round(h * max(ratio)))
    else:
        w, h = width, height
    h, w = max(1, min(h, height)), max(1, min(w, width))
    return (height - h) // 2, (width - w) // 2, h, w


def _jitter_ranges(color_jitter):
    """ColorJitter's (brightness, contrast, saturation) ranges [max(0, 1 - v), 1 + v]; None where the op is off."""
    if color_jitter is None:
        return None
    if isinstance(color_jitter, (list, tuple)):
        if len(color_jitter) not in (3, 4):
            raise ValueError('color_jitter: a number or 3 values (brightness, contrast, saturation)')
        if len(color_jitter) == 4 and color_jitter[3]:
            raise NotImplementedError('color_jitter: hue is not built')
        vals = [float(v) for v in color_jitter[:3]]
    else:
        vals = [float(color_jitter)] * 3
    out = []
    for v in vals:
        if v < 0:
            raise ValueError('color_jitter: values must be non-negative')
        out.append(None if v == 0 else (max(0.0, 1.0 - v), 1.0 + v))
    return out


def _randaug_magnitudes(out_hw, magnitude, bins):
    """RandAugment._augmentation_space at one bin: the magnitude of each of the 14 ops for (height, width) frames (float32
    linspaces read with float(), as torchvision does)."""
    H, W = int(out_hw[0]), int(out_hw[1])
    at = lambda lo, hi: float(torch.linspace(lo, hi, bins)[magnitude])
    shear, colour = at(0.0, 0.3), at(0.0, 0.9)
    posterize = float((8 - (torch.arange(bins) / ((bins - 1) / 4)).round().int())[magnitude])
    return (0.0, shear, shear, at(0.0, 150.0 / 331.0 * W), at(0.0, 150.0 / 331.0 * H), at(0.0, 30.0), colour, colour, colour, colour,
            posterize, at(255.0, 0.0), 0.0, 0.0)


def _draw_randaug(mags, num_ops, generator):
    """RandAugment.forward's draws for one clip: per op randint(14), and randint(2) for the sign if the op is signed."""
    rec = []
    for _ in range(num_ops):
        op = int(torch.randint(len(RANDAUG_OPS), (1,), generator=generator))
        mag = mags[op]
        if op in _RA_SIGNED and int(torch.randint(2, (1,), generator=generator)):
            mag *= -1.0
        rec.append((op, mag))
    return tuple(rec)


def sample_randaug(B, out_hw, num_ops=2, magnitude=9, num_magnitude_bins=31, generator=None):
    """The draws of torchvision's RandAugment(num_ops, magnitude, num_magnitude_bins) for B clips of ``out_hw`` = (height, width)
    frames (the size RandAugment sees: it runs behind the crop): per clip a tuple of (op index into RANDAUG_OPS, signed magnitude)
    in the order of application.  One draw per clip: every frame shares it."""
    num_ops, magnitude, bins = int(num_ops), int(magnitude), int(num_magnitude_bins)
    if num_ops < 0 or bins < 2 or not 0 <= magnitude < bins:
        raise ValueError(f'sample_randaug: num_ops={num_ops} >= 0, 0 <= magnitude={magnitude} < num_magnitude_bins={bins} expected')
    mags = _randaug_magnitudes(out_hw, magnitude, bins)
    return [_draw_randaug(mags, num_ops, generator) for _ in range(int(B))]


def _inverse_affine(center, angle, translate, shear):
    """torchvision's _get_inverse_affine_matrix at scale 1 (degrees in, float64)."""
    rot, sx, sy = math.radians(angle), math.radians(shear[0]), math.radians(shear[1])
    cx, cy = center
    tx, ty = translate
    a = math.cos(rot - sy) / math.cos(sy)
    b = -math.cos(rot - sy) * math.tan(sx) / math.cos(sy) - math.sin(rot)
    c = math.sin(rot - sy) / math.cos(sy)
    d = -math.sin(rot - sy) * math.tan(sx) / math.cos(sy) + math.cos(rot)
    m = [d, -b, 0.0, -c, a, 0.0]
    m[2] += m[0] * (-cx - tx) + m[1] * (-cy - ty)
    m[5] += m[3] * (-cx - tx) + m[4] * (-cy - ty)
    m[2] += cx
    m[5] += cy
    return m


def randaug_theta(op, mag, H, W):
    """The six entries of the inverse matrix RandAugment._apply_op hands to the warp for a geometric op (1 .. 5) of signed magnitude
    ``mag`` on H x W frames: shear about center=[0, 0] (the frame's corner, (-W/2, -H/2) from its middle), translation by int(mag)
    pixels, rotation by ``mag`` degrees through F.rotate (angle -mag)."""
    if op in (1, 2):
        sh = math.degrees(math.atan(mag))
        return _inverse_affine((-W * 0.5, -H * 0.5), 0.0, (0.0, 0.0), (sh, 0.0) if op == 1 else (0.0, sh))
    if op in (3, 4):
        return _inverse_affine((0.0, 0.0), 0.0, (float(int(mag)), 0.0) if op == 3 else (0.0, float(int(mag))), (0.0, 0.0))
    if op == 5:
        return _inverse_affine((0.0, 0.0), -mag, (0.0, 0.0), (0.0, 0.0))
    raise ValueError(f'randaug_theta: op {op} is not geometric')


def sample_params(B, src_hw, scale=None, ratio=None, hflip=0.5, color_jitter=0.4, generator=None, auto_augment=None, out_hw=None):
    """The draws of RandomResizedCrop + RandomHorizontalFlip + ColorJitter for B clips of ``src_hw`` = (height, width) frames, or
    of B clips of their own sizes, ``src_hw`` = B pairs (height, width) -- the draws are then those of B successive one-clip calls
    on the same generator: a list of B ``ClipDraw``.  Host code; all randomness comes from ``generator`` (None = torch's default CPU generator).
    A truthy ``auto_augment`` draws RandAugment() for ``out_hw`` frames in place of the ColorJitter (``ops`` and ``factors`` stay
    empty), clip by clip: crop, flip, RandAugment."""
    if np.ndim(src_hw) == 2:
        sizes = [(int(h), int(w)) for h, w in src_hw]
        if len(sizes) != int(B):
            raise ValueError(f'sample_params: {len(sizes)} frame sizes for {B} clips')
    else:
        sizes = [(int(src_hw[0]), int(src_hw[1]))] * int(B)
    scale = tuple(scale or (0.08, 1.0))
    ratio = tuple(ratio or (3. / 4., 4. / 3.))
    ranges = _jitter_ranges(color_jitter)
    mags = None
    if auto_augment:
        if out_hw is None:
            raise ValueError('sample_params: auto_augment needs out_hw, the frame size behind the crop')
        ranges, mags = None, _randaug_magnitudes(out_hw, 9, 31)
    draws = []
    for height, width in sizes:
        top, left, h, w = _crop_box(height, width, scale, ratio, generator)
        flip = bool(hflip > 0. and float(torch.rand(1, generator=generator)) < hflip)
        jops, jfac = [], []
        if ranges is not None:
            order = torch.randperm(4, generator=generator).tolist()          # ColorJitter.get_params: the order, then b, c, s
            fac = [None if r is None else _uniform(r[0], r[1], generator) for r in ranges]
            for fn in order:
                if fn < 3 and fac[fn] is not None:
                    jops.append(fn)
                    jfac.append(fac[fn])
        draws.append(ClipDraw(top, left, h, w, flip, tuple(jops), tuple(jfac), _draw_randaug(mags, 2, generator) if mags else ()))
    return draws


def _check_draws(draws, B, Hs, Ws, num_ops=2):
    """Hs, Ws: the frame size of every clip, or B sizes each (a list of clips)."""
    if len(draws) != B:
        raise ValueError(f'params: {len(draws)} records for {B} clips')
    sizes = zip(Hs, Ws) if isinstance(Hs, (list, tuple)) else [(Hs, Ws)] * B
    for d, (Hs, Ws) in zip(draws, sizes):
        if not (0 <= d.top and 0 < d.height and d.top + d.height <= Hs and 0 <= d.left and 0 < d.width and d.left + d.width <= Ws):
            raise ValueError(f'params: crop box (top {d.top}, left {d.left}, {d.height}x{d.width}) outside the {Hs}x{Ws} frame')
        if len(d.ops) != len(d.factors) or len(d.ops) > 3 or len(set(d.ops)) != len(d.ops) or any(o not in (0, 1, 2) for o in d.ops):
            raise ValueError(f'params: colour ops {d.ops} / factors {d.factors}: each of 0, 1, 2 at most once, one factor per op')
        ra = d.randaug
        if len(ra) > num_ops or (ra and d.ops):
            raise ValueError(f'params: RandAugment record {ra}: at most {num_ops} ops, and none beside colour-jitter ops')
        for rec in ra:
            if (len(rec) != 2 or isinstance(rec[0], bool) or not isinstance(rec[0], (int, np.integer)) or not 0 <= rec[0] < len(RANDAUG_OPS)
                    or not math.isfinite(rec[1])):
                raise ValueError(f'params: RandAugment record {rec}: (op index 0 .. {len(RANDAUG_OPS) - 1}, finite magnitude)')


def _tables(specs, mode, antialias):
    """specs: per clip (src_len, crop_start, crop_len, out_len, flip, lo, n) -> first [B,n], count [B,n], weights [B,n,taps]
    (rows lo .. lo+n of each clip's table; where n differs between the clips, the largest, and the shorter tables end in rows of
    count 0)."""
    taps = max(ops.resample_max_taps(s[2], s[3], mode, antialias) for s in specs)
    built = {}                                              # clips that share a spec (ClipEval: all of them) share the table
    for s in specs:
        if s[:5] not in built:
            built[s[:5]] = ops.resample_table(s[0], s[1], s[2], s[3], mode, antialias, s[4], taps)
    tabs = [built[s[:5]] for s in specs]
    cut = [tuple(a[s[5]:s[5] + s[6]] for a in t) for t, s in zip(tabs, specs)]
    n = max(s[6] for s in specs)
    if any(s[6] != n for s in specs):
        cut = [tuple(np.concatenate([a, np.zeros((n - len(a),) + a.shape[1:], dtype=a.dtype)]) for a in c) for c in cut]
    return tuple(np.stack([c[i] for c in cut]) for i in range(3))


def _randaug_plan(draws, H, W):
    """The launches of the RandAugment records, slot by slot: [(kernel family, [host records])].  Within a slot every clip drew one
    op, so the batch splits by family and each family needed is launched once, with ``sel`` (or per-clip records) naming the
    clips that drew it; Identity launches nothing."""
    B = len(draws)
    plan = []
    for s in range(max(len(d.randaug) for d in draws)):
        theta = np.tile(np.array([1, 0, 0, 0, 1, 0], dtype=np.float32), (B, 1))
        sharp, jf = np.zeros((B, 2), dtype=np.float32), np.zeros((B, 6), dtype=np.float32)
        jo, pw = np.zeros((B, 4), dtype=np.int32), np.zeros((B, 2), dtype=np.int32)
        sel = {k: np.zeros(B, dtype=np.int32) for k in ('warp', 'sharpness', 'autocontrast', 'equalize')}
        for b, d in enumerate(draws):
            if s >= len(d.randaug):
                continue
            op, mag = int(d.randaug[s][0]), float(d.randaug[s][1])
            if 1 <= op <= 5:
                theta[b], sel['warp'][b] = randaug_theta(op, mag, H, W), 1
            elif op in _RA_JITTER:
                jo[b, :2] = (1, _RA_JITTER[op])
                jf[b, 0], jf[b, 3] = 1.0 + mag, 1.0 - (1.0 + mag)                # 1 - r in float64, then rounded: torchvision's _blend
            elif op == 9:
                sharp[b], sel['sharpness'][b] = (1.0 + mag, 1.0 - (1.0 + mag)), 1
            elif op == 10:
                pw[b] = (1, int(mag))
            elif op == 11:
                pw[b] = (2, math.ceil(mag))                                     # v >= 178.5 for integers: v >= 179
            elif op == 12:
                sel['autocontrast'][b] = 1
            elif op == 13:
                sel['equalize'][b] = 1
        if sel['warp'].any():
            plan.append(('warp', [theta, sel['warp']]))
        if sel['sharpness'].any():
            plan.append(('sharpness', [sharp, sel['sharpness']]))
        if jo.any():
            plan.append(('jitter', [jo, jf]))
        if pw.any():
            plan.append(('pointwise', [pw]))
        for k in ('autocontrast', 'equalize'):
            if sel[k].any():
                plan.append((k, [sel[k]]))
    return plan


def _run(clips, xspecs, yspecs, out_hw, mode, antialias, draws=None, frames=None, lefts=None):
    """Tables (and colour / RandAugment records) to the device in one copy, then the kernels.  With ``frames`` (int32 [B,T]) or
    ``lefts`` (int32 [B,V]: the x tables then cover the whole resized row and out_hw[1] is the width of a view) the resampling is
    clip_views_u8's, and its [B,V,T,H,W,3] is returned as [B*V,T,H,W,3].  ``clips`` a list: clips_views_u8's, always (of YUVClip:
    clips_views_yuv's); the pointer table and geometry travel at the front of the same copy (the x table of clip b holds
    xspecs[b][6] columns)."""
    ragged = isinstance(clips, (list, tuple))
    xf, xc, xw = _tables(xspecs, mode, antialias)
    yf, yc, yw = _tables(yspecs, mode, antialias)
    parts = [xf, xc, xw.view(np.int32), yf, yc, yw.view(np.int32)]
    jitter = draws is not None and any(d.ops for d in draws)
    if jitter:
        B = len(draws)
        jo = np.zeros((B, 4), dtype=np.int32)
        jf = np.zeros((B, 6), dtype=np.float32)
        for b, d in enumerate(draws):
            jo[b, 0] = len(d.ops)
            jo[b, 1:1 + len(d.ops)] = d.ops
            jf[b, :len(d.ops)] = d.factors
            jf[b, 3:3 + len(d.ops)] = [1.0 - float(f) for f in d.factors]      # in float64, then rounded: torchvision's _blend
        parts += [jo, jf.view(np.int32)]
    plan = _randaug_plan(draws, out_hw[0], out_hw[1]) if draws is not None and any(d.randaug for d in draws) else []
    for _, recs in plan:
        parts += [r.view(np.int32) for r in recs]
    gather = ragged or frames is not None or lefts is not None
    if gather:
        if lefts is None:
            lefts = np.zeros((len(xspecs), 1), dtype=np.int32)
        parts += [lefts] + ([frames] if frames is not None else [])
    if ragged:                                               # every check of the list happens here, before anything is enqueued
        clips = ops.clips_table(clips, [s[6] for s in xspecs], 'vtx.aug')
        parts.insert(0, clips.host)                          # first: the 8-byte pointers are aligned there
    dev = ops.upload_i32(np.concatenate([p.reshape(-1) for p in parts]), clips.device)
    views, at = [], 0
    for p in parts:
        views.append(dev[at:at + p.size].view(p.shape))
        at += p.size
    if ragged:
        parts, table = parts[1:], views.pop(0)
    f32 = lambda t: t.view(torch.float32)
    xtab, ytab = (views[0], views[1], f32(views[2])), (views[3], views[4], f32(views[5]))
    if gather:
        at = len(parts) - (1 if frames is None else 2)
        if ragged:
            views_of = ops.clips_views_yuv if clips.yuv else ops.clips_views_u8
            out = views_of(clips, None if frames is None else views[at + 1], views[at], out_hw[1], xtab, ytab, table=table)
        else:
            out = ops.clip_views_u8(clips, None if frames is None else views[at + 1], views[at], out_hw[1], xtab, ytab)
        out = out.view((-1,) + tuple(out.shape[2:]))
    else:
        out = ops.clip_resample_u8(clips, out_hw, xtab, ytab)
    if jitter:
        ops.clip_jitter_u8_(out, views[6], f32(views[7]))
    at = 8 if jitter else 6
    for kind, recs in plan:
        v = views[at:at + len(recs)]
        at += len(recs)
        if kind == 'warp':
            out = ops.clip_warp_nearest_u8(out, f32(v[0]), v[1])
        elif kind == 'sharpness':
            out = ops.clip_sharpness_u8(out, f32(v[0]), v[1])
        elif kind == 'jitter':
            ops.clip_jitter_u8_(out, v[0], f32(v[1]))
        elif kind == 'pointwise':
            ops.clip_pointwise_u8_(out, v[0])
        elif kind == 'autocontrast':
            ops.clip_autocontrast_u8_(out, v[0])
        else:
            ops.clip_equalize_u8_(out, v[0])
    return out


def _check_clips(clips):
    ops._check_u8_clip(clips, 'vtx.aug')
    return clips.shape[0], clips.shape[2], clips.shape[3]


def _check_clip_list(clips, frames):
    """A list of clips [Ts_b,Hs_b,Ws_b,3] (or of YUVClip) and its frames= -> (B, [Hs_b], [Ws_b], int32 frames [B,T] or None).  Host checks of types,
    shapes and indices; where the tensors live is checked with everything else before the upload (ops.clips_table)."""
    shapes = ops.clip_list_shapes(clips, 'vtx.aug')
    frames = _check_frames_ragged(frames, [s[0] for s in shapes])
    return len(shapes), [s[1] for s in shapes], [s[2] for s in shapes], frames


class ClipAugment:
    """``transforms_train`` (data_transform.py:495-531) without its ToTensor + Normalize tail, per clip on the device.  Takes
    that function's arguments and defaults; ``scale=(0.5, 1.0), color_jitter=None`` is the ``mim`` branch of
    data_trainer.py:61-63; a truthy ``auto_augment`` (the -auto_augment flag, data_trainer.py:82) puts RandAugment() in the place
    of the ColorJitter, whatever the string says.  uint8 CUDA [B,T,Hs,Ws,3], or a list of B uint8 CUDA clips [Ts_b,Hs_b,Ws_b,3] of
    their own sizes, or a list of B ``vtx.YUVClip`` (decoded 4:2:0 planes), -> uint8 CUDA [B,T,img_size,img_size,3]."""

    def __init__(self, img_size=224, scale=None, ratio=None, hflip=0.5, color_jitter=0.4, interpolation='bicubic', antialias=False,
                 auto_augment=None):
        self.auto_augment = auto_augment
        self.out_hw = (int(img_size), int(img_size)) if not isinstance(img_size, (tuple, list)) else (int(img_size[0]), int(img_size[1]))
        self.scale, self.ratio, self.hflip, self.color_jitter = scale, ratio, float(hflip), color_jitter
        ops._resample_mode(interpolation)
        _jitter_ranges(color_jitter)
        self.interpolation, self.antialias = interpolation, bool(antialias)

    def __call__(self, clips_u8, generator=None, params=None, frames=None):
        """``frames``: host integers [B,T] (or [T] for every clip alike), the decoded frames to take (``sample_frames``); the result
        is that of the call on ``clips_u8[b, frames[b]]`` under the same draws, without the gathered copy.  A list of clips: row b
        of ``frames`` indexes its own clip's frames, and clip b's result is that of the call on ``clips_u8[b][None]`` with
        ``params[b]`` and ``frames[b]``; without ``frames`` the clips must agree in length."""
        if isinstance(clips_u8, (list, tuple)):
            B, Hs, Ws, frames = _check_clip_list(clips_u8, frames)
            if params is None:
                params = sample_params(B, list(zip(Hs, Ws)), self.scale, self.ratio, self.hflip, self.color_jitter, generator,
                                       auto_augment=self.auto_augment, out_hw=self.out_hw)
            _check_draws(params, B, Hs, Ws)
            H, W = self.out_hw
            xs = [(w, d.left, d.width, W, d.flip, 0, W) for d, w in zip(params, Ws)]
            ys = [(h, d.top, d.height, H, False, 0, H) for d, h in zip(params, Hs)]
            return _run(clips_u8, xs, ys, self.out_hw, self.interpolation, self.antialias, params, frames=frames)
        B, Hs, Ws = _check_clips(clips_u8)
        if frames is not None:
            frames = _check_frames(frames, B, clips_u8.shape[1])
        if params is None:
            params = sample_params(B, (Hs, Ws), self.scale, self.ratio, self.hflip, self.color_jitter, generator,
                                   auto_augment=self.auto_augment, out_hw=self.out_hw)
        _check_draws(params, B, Hs, Ws)
        H, W = self.out_hw
        xs = [(Ws, d.left, d.width, W, d.flip, 0, W) for d in params]
        ys = [(Hs, d.top, d.height, H, False, 0, H) for d in params]
        return _run(clips_u8, xs, ys, self.out_hw, self.interpolation, self.antialias, params, frames=frames)


class ClipEval:
    """``transforms_eval`` (data_transform.py:546-566) without ToTensor + Normalize: resize the short side to
    floor(img_size / crop_pct), centre crop img_size -- one resampling pass whose tables are those of the whole resized frame,
    cut to the crop window."""

    def __init__(self, img_size=224, crop_pct=None, interpolation='bicubic', antialias=False):
        self.img_size = int(img_size)
        self.scale_size = int(math.floor(self.img_size / (crop_pct or 0.875)))
        ops._resample_mode(interpolation)
        self.interpolation, self.antialias = interpolation, bool(antialias)

    def resized_hw(self, Hs, Ws):
        """torchvision Resize(int): the short side becomes scale_size, the long side int(scale_size * long / short)."""
        short, long = (Ws, Hs) if Ws <= Hs else (Hs, Ws)
        new_short, new_long = self.scale_size, int(self.scale_size * long / short)
        return (new_long, new_short) if Ws <= Hs else (new_short, new_long)

    def __call__(self, clips_u8, frames=None):
        """``frames``: as ClipAugment's.  A list of clips: each is resized and cropped by its own size."""
        S = self.img_size
        if isinstance(clips_u8, (list, tuple)):
            B, Hs, Ws, frames = _check_clip_list(clips_u8, frames)
            xs, ys = [], []
            for b in range(B):
                Hr, Wr = self.resized_hw(Hs[b], Ws[b])
                if Hr < S or Wr < S:
                    raise ValueError(f'ClipEval: the resized frame {Hr}x{Wr} of clip {b} ({Hs[b]}x{Ws[b]}) is smaller than the {S}x{S} crop '
                                     '(padding is not built)')
                xs.append((Ws[b], 0, Ws[b], Wr, False, int(round((Wr - S) / 2.0)), S))
                ys.append((Hs[b], 0, Hs[b], Hr, False, int(round((Hr - S) / 2.0)), S))
            return _run(clips_u8, xs, ys, (S, S), self.interpolation, self.antialias, frames=frames)
        B, Hs, Ws = _check_clips(clips_u8)
        if frames is not None:
            frames = _check_frames(frames, B, clips_u8.shape[1])
        Hr, Wr = self.resized_hw(Hs, Ws)
        S = self.img_size
        if Hr < S or Wr < S:
            raise ValueError(f'ClipEval: the resized frame {Hr}x{Wr} is smaller than the {S}x{S} crop (padding is not built)')
        top, left = int(round((Hr - S) / 2.0)), int(round((Wr - S) / 2.0))
        xs = [(Ws, 0, Ws, Wr, False, left, S)] * B
        ys = [(Hs, 0, Hs, Hr, False, top, S)] * B
        return _run(clips_u8, xs, ys, (S, S), self.interpolation, self.antialias, frames=frames)


class ClipTest:
    """The reference's test pipeline (data_trainer.py:108-121) without ToTensor + Normalize: ``Resize(short side short_side)``, then
    ``ThreeCrop(img_size)`` (data_transform.py:412-461) -- three img_size x img_size windows of the resized frame that share the
    rows from (Hr - S) // 2 and begin at columns 0, Wr - S and (Wr - S) // 2: left, right, centre, the order the reference stacks
    them in.  One launch: each column of the resized frame that a window holds is resampled once, with the tables of the whole
    resized frame, and stored to every window that holds it.  uint8 CUDA [B,Ts,Hs,Ws,3] -> uint8 CUDA [B*3,T,S,S,3], view v of clip
    b in row b*3 + v: what ``test_step``'s ``preds.view(-1, n_crops, num_class).mean(1)`` averages.  (The reference's own collate
    yields [B,3,T,C,H,W], which its models cannot take; ``test_step`` here flattens such a batch.)

    ``interpolation='bilinear'`` is the default of the torchvision ``Resize`` the pipeline calls.  ``antialias``: torchvision's
    default for tensors changed between versions (off up to 0.16, on from 0.17), so it is an argument here; torchvision is not a
    dependency and no version is pinned."""
    n_crops = 3

    def __init__(self, img_size=224, short_side=256, interpolation='bilinear', antialias=False):
        self.img_size, self.short_side = int(img_size), int(short_side)
        if self.img_size < 1 or self.short_side < 1:
            raise ValueError(f'ClipTest: img_size={img_size} and short_side={short_side} must be positive')
        ops._resample_mode(interpolation)
        self.interpolation, self.antialias = interpolation, bool(antialias)

    def resized_hw(self, Hs, Ws):
        """torchvision Resize(int): the short side becomes short_side, the long side int(short_side * long / short)."""
        short, long = (Ws, Hs) if Ws <= Hs else (Hs, Ws)
        new_short, new_long = self.short_side, int(self.short_side * long / short)
        return (new_long, new_short) if Ws <= Hs else (new_short, new_long)

    def offsets(self, Hs, Ws):
        """-> (top, (left, right, centre) first columns) of the three windows in the resized frame."""
        Hr, Wr = self.resized_hw(Hs, Ws)
        S = self.img_size
        if S > Hr or S > Wr:
            raise ValueError('Requested crop size {} is bigger than input size {}'.format(S, (Hr, Wr)))
        return (Hr - S) // 2, (0, Wr - S, (Wr - S) // 2)

    def specs(self, sizes):
        """For clips of ``sizes`` = [(Hs_b, Ws_b)]: -> (x specs, y specs, lefts int32 [B,3]) of ``_tables`` / ``_run``.  The x table of
        clip b has the Wr_b columns of its own resized row; ``_tables`` pads them to the widest with count 0."""
        S = self.img_size
        xs, ys, lefts = [], [], []
        for b, (Hs, Ws) in enumerate(sizes):
            Hr, Wr = self.resized_hw(Hs, Ws)
            try:
                top, left = self.offsets(Hs, Ws)
            except ValueError as e:
                raise ValueError(f'{e} (clip {b}, {Hs}x{Ws})') from None
            xs.append((Ws, 0, Ws, Wr, False, 0, Wr))
            ys.append((Hs, 0, Hs, Hr, False, top, S))
            lefts.append(left)
        return xs, ys, np.array(lefts, dtype=np.int32)

    def __call__(self, clips_u8, frames=None):
        """``frames``: as ClipAugment's; None takes every frame.  A list of clips: each is resized and cropped by its own size, view
        v of clip b in row b*3 + v as ever."""
        if isinstance(clips_u8, (list, tuple)):
            B, Hs, Ws, frames = _check_clip_list(clips_u8, frames)
            xs, ys, lefts = self.specs(list(zip(Hs, Ws)))
            return _run(clips_u8, xs, ys, (self.img_size, self.img_size), self.interpolation, self.antialias, frames=frames, lefts=lefts)
        B, Hs, Ws = _check_clips(clips_u8)
        if frames is not None:
            frames = _check_frames(frames, B, clips_u8.shape[1])
        Hr, Wr = self.resized_hw(Hs, Ws)
        top, lefts = self.offsets(Hs, Ws)
        S = self.img_size
        xs = [(Ws, 0, Ws, Wr, False, 0, Wr)] * B
        ys = [(Hs, 0, Hs, Hr, False, top, S)] * B
        return _run(clips_u8, xs, ys, (S, S), self.interpolation, self.antialias, frames=frames,
                    lefts=np.tile(np.array(lefts, dtype=np.int32), (B, 1)))
