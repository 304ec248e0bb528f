"""CPU restatement of torchvision's RandAugment ops (tensor path, 0.13 .. 0.20; torchvision itself is not a dependency and no
version is pinned) for tests/test_randaug_host.py and tests/test_gpu_randaug.py.  No tests here.

``apply_op`` is autoaugment._apply_op on a uint8 [T,H,W,3] clip with RandAugment's defaults (nearest, fill None) in plain torch:
the warp goes through F.grid_sample as functional_tensor._apply_grid_transform does it, the sharpness through F.conv2d, the
colour ops through aug_ref's blends.  ``warp_coords64`` is the same warp's source coordinate in float64, with ``near_tie`` the
pixels whose coordinate lies within TIE of a rounding tie, where a float32 evaluation may pick the other neighbour.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

import aug_ref as A

OPS = ('Identity', 'ShearX', 'ShearY', 'TranslateX', 'TranslateY', 'Rotate', 'Brightness', 'Color', 'Contrast', 'Sharpness',
       'Posterize', 'Solarize', 'AutoContrast', 'Equalize')
SIGNED = tuple(range(1, 10))
GEOMETRIC = (1, 2, 3, 4, 5)
TIE = 1e-3           # |frac(coordinate) - 0.5| below which either neighbour is accepted (float32 coordinates of ~1e2: error ~1e-5)
TIE_SHARE = 0.02     # at most this share of a case's pixels may be that close (measured: <= 0.0054, Rotate only)
SHAPES = [(40, 56), (33, 47)]       # 2240 pixels: the word path; 1551 pixels, odd rows: the byte path


def magnitudes(hw, bin_=9, bins=31):
    """RandAugment._augmentation_space((H, W)) at one bin, op by op."""
    H, W = hw
    at = lambda lo, hi: float(torch.linspace(lo, hi, bins)[bin_])
    post = float((8 - (torch.arange(bins) / ((bins - 1) / 4)).round().int())[bin_])
    return [0.0, at(0.0, 0.3), at(0.0, 0.3), at(0.0, 150.0 / 331.0 * W), at(0.0, 150.0 / 331.0 * H), at(0.0, 30.0), at(0.0, 0.9),
            at(0.0, 0.9), at(0.0, 0.9), at(0.0, 0.9), post, at(255.0, 0.0), 0.0, 0.0]


def signed_cases(hw):
    """(op, magnitude) for every geometric op in both signs: the ten warp cases."""
    m = magnitudes(hw)
    return [(op, s * m[op]) for op in GEOMETRIC for s in (1.0, -1.0)]


def _inverse_affine_matrix(center, angle, translate, scale, shear):
    rot = math.radians(angle)
    sx = math.radians(shear[0])
    sy = math.radians(shear[1])
    cx, cy = center
    tx, ty = translate
    a = math.cos(rot - sy) / math.cos(sy)
    b = -math.cos(rot - sy) * math.tan(sx) / math.cos(sy) - math.sin(rot)
    c = math.sin(rot - sy) / math.cos(sy)
    d = -math.sin(rot - sy) * math.tan(sx) / math.cos(sy) + math.cos(rot)
    matrix = [d, -b, 0.0, -c, a, 0.0]
    matrix = [x / scale for x in matrix]
    matrix[2] += matrix[0] * (-cx - tx) + matrix[1] * (-cy - ty)
    matrix[5] += matrix[3] * (-cx - tx) + matrix[4] * (-cy - ty)
    matrix[2] += cx
    matrix[5] += cy
    return matrix


def matrix_of(op, mag, hw):
    """The matrix F.affine / F.rotate compute for _apply_op's arguments (tensor input: the centre is relative to the middle)."""
    H, W = hw
    corner = [1.0 * (c - s * 0.5) for c, s in zip([0, 0], [W, H])]         # center=[0, 0] of the shears
    if op == 1:
        return _inverse_affine_matrix(corner, 0.0, [0.0, 0.0], 1.0, [math.degrees(math.atan(mag)), 0.0])
    if op == 2:
        return _inverse_affine_matrix(corner, 0.0, [0.0, 0.0], 1.0, [0.0, math.degrees(math.atan(mag))])
    if op == 3:
        return _inverse_affine_matrix([0.0, 0.0], 0.0, [1.0 * int(mag), 0.0], 1.0, [0.0, 0.0])
    if op == 4:
        return _inverse_affine_matrix([0.0, 0.0], 0.0, [0.0, 1.0 * int(mag)], 1.0, [0.0, 0.0])
    if op == 5:
        return _inverse_affine_matrix([0.0, 0.0], -mag, [0.0, 0.0], 1.0, [0.0, 0.0])
    raise ValueError(op)


def _nchw(frames_u8):
    return frames_u8.permute(0, 3, 1, 2).contiguous()


def _nhwc(img):
    return img.permute(0, 2, 3, 1).contiguous()


def warp_grid_sample(frames_u8, matrix):
    """functional_tensor.affine / rotate: _gen_affine_grid in float32, grid_sample nearest, zeros, align_corners=False."""
    img = _nchw(frames_u8)
    n, _, h, w = img.shape
    theta = torch.tensor(matrix, dtype=torch.float32).reshape(1, 2, 3)
    d = 0.5
    base = torch.empty(1, h, w, 3, dtype=torch.float32)
    base[..., 0].copy_(torch.linspace(-w * 0.5 + d, w * 0.5 + d - 1, steps=w))
    base[..., 1].copy_(torch.linspace(-h * 0.5 + d, h * 0.5 + d - 1, steps=h).unsqueeze_(-1))
    base[..., 2].fill_(1)
    rescaled = theta.transpose(1, 2) / torch.tensor([0.5 * w, 0.5 * h], dtype=torch.float32)
    grid = base.view(1, h * w, 3).bmm(rescaled).view(1, h, w, 2)
    out = F.grid_sample(img.float(), grid.expand(n, h, w, 2), mode='nearest', padding_mode='zeros', align_corners=False)
    return _nhwc(torch.round(out).to(torch.uint8))


def warp_coords64(matrix, hw):
    """float64 (sx, sy) [H,W] of the source coordinate of every output pixel."""
    H, W = hw
    m = [float(v) for v in np.asarray(matrix, dtype=np.float32)]           # the matrix as the float32 tensor holds it
    xo = np.arange(W, dtype=np.float64)[None, :] - W / 2 + 0.5
    yo = np.arange(H, dtype=np.float64)[:, None] - H / 2 + 0.5
    sx = m[0] * xo + m[1] * yo + m[2] + W / 2 - 0.5
    sy = m[3] * xo + m[4] * yo + m[5] + H / 2 - 0.5
    return sx, sy


def _tie(v):
    return np.abs(np.abs(v - np.floor(v)) - 0.5) < TIE


def near_tie(sx, sy):
    return _tie(sx) | _tie(sy)


def _take(frames, ix, iy):
    """frames uint8 [T,H,W,3] (NumPy) at integer coordinates [H,W], 0 outside."""
    T, H, W, _ = frames.shape
    ok = (ix >= 0) & (ix < W) & (iy >= 0) & (iy < H)
    out = frames[:, np.clip(iy, 0, H - 1), np.clip(ix, 0, W - 1)]
    out[:, ~ok] = 0
    return out


def warp_float64(frames_u8, matrix):
    """The float64 form: source pixel at (rint sx, rint sy), halves to even, 0 outside -> uint8 [T,H,W,3] (NumPy)."""
    f = np.asarray(frames_u8)
    sx, sy = warp_coords64(matrix, f.shape[1:3])
    return _take(f, np.rint(sx).astype(np.int64), np.rint(sy).astype(np.int64))


def warp_matches(got_u8, frames_u8, matrix):
    """[H,W] bool: the pixel (all frames, all channels) equals the float64 form, or, within near_tie, one of the candidate source
    pixels (floor or ceil on each coordinate that is near a tie)."""
    f, g = np.asarray(frames_u8), np.asarray(got_u8)
    sx, sy = warp_coords64(matrix, f.shape[1:3])
    tx, ty = _tie(sx), _tie(sy)
    ok = np.zeros(sx.shape, dtype=bool)
    for cx in (np.floor, np.ceil):
        for cy in (np.floor, np.ceil):
            ix = np.where(tx, cx(sx), np.rint(sx)).astype(np.int64)
            iy = np.where(ty, cy(sy), np.rint(sy)).astype(np.int64)
            ok |= np.all(_take(f, ix, iy) == g, axis=(0, 3))
    return ok


def sharpness(frames_u8, factor):
    """adjust_sharpness: _blurred_degenerate_image (float32 conv2d, round, cast; the border is the image) and _blend."""
    img = _nchw(frames_u8)
    if img.size(-1) <= 2 or img.size(-2) <= 2:
        return frames_u8.clone()
    kernel = torch.ones((3, 3), dtype=torch.float32)
    kernel[1, 1] = 5.0
    kernel /= kernel.sum()
    kernel = kernel.expand(3, 1, 3, 3)
    blurred = torch.round(F.conv2d(img.float(), kernel, groups=3)).to(torch.uint8)
    degenerate = img.clone()
    degenerate[..., 1:-1, 1:-1] = blurred
    return _nhwc(A._blend(img, degenerate, factor))


def posterize(frames_u8, bits):
    return frames_u8 & (-int(2 ** (8 - int(bits))) & 255)


def solarize(frames_u8, threshold):
    return torch.where(frames_u8 >= threshold, 255 - frames_u8, frames_u8)


def autocontrast(frames_u8):
    img = _nchw(frames_u8)
    minimum = img.amin(dim=(-2, -1), keepdim=True).to(torch.float32)
    maximum = img.amax(dim=(-2, -1), keepdim=True).to(torch.float32)
    scale = 255.0 / (maximum - minimum)
    eq = torch.isfinite(scale).logical_not()
    minimum[eq] = 0
    scale[eq] = 1
    return _nhwc(((img - minimum) * scale).clamp(0, 255).to(torch.uint8))


def _scale_channel(chan):
    hist = torch.bincount(chan.reshape(-1).long(), minlength=256)
    nonzero = hist[hist != 0]
    step = torch.div(nonzero[:-1].sum(), 255, rounding_mode='floor')
    if step == 0:
        return chan
    lut = torch.div(torch.cumsum(hist, 0) + torch.div(step, 2, rounding_mode='floor'), step, rounding_mode='floor')
    lut = F.pad(lut, [1, 0])[:-1].clamp(0, 255)
    return lut[chan.long()].to(torch.uint8)


def equalize(frames_u8):
    img = _nchw(frames_u8)
    return _nhwc(torch.stack([torch.stack([_scale_channel(img[t, c]) for c in range(3)]) for t in range(img.shape[0])]))


def apply_op(frames_u8, op, mag):
    """autoaugment._apply_op on uint8 [T,H,W,3] -> uint8 [T,H,W,3] (torch)."""
    if op == 0:
        return frames_u8.clone()
    if op in GEOMETRIC:
        return warp_grid_sample(frames_u8, matrix_of(op, mag, tuple(frames_u8.shape[1:3])))
    if op in (6, 7, 8):
        return A.jitter_ref(frames_u8, [{6: 0, 7: 2, 8: 1}[op]], [1.0 + mag])
    if op == 9:
        return sharpness(frames_u8, 1.0 + mag)
    if op == 10:
        return posterize(frames_u8, int(mag))
    if op == 11:
        return solarize(frames_u8, mag)
    if op == 12:
        return autocontrast(frames_u8)
    if op == 13:
        return equalize(frames_u8)
    raise ValueError(op)


def planted_clip(hw, seed):
    """uint8 [3,2,H,W,3]: aug_ref.source_clip (frame [0,0] all 0, frame [1,1] all 255) with three more planted frames:
    [0,1] holds only the values 100 .. 110; [1,0] is 255 but for 200 pixels (equalize: step == 0); [2,0] has a constant green
    channel (autocontrast: hi == lo on that channel only)."""
    clip = A.source_clip(3, 2, hw, seed)
    g = torch.Generator().manual_seed(seed + 1000)
    H, W = hw
    clip[0, 1] = torch.randint(100, 111, (H, W, 3), generator=g, dtype=torch.uint8)
    frame = torch.full((H * W, 3), 255, dtype=torch.uint8)
    at = torch.randperm(H * W, generator=g)[:200]
    frame[at] = torch.randint(0, 255, (200, 3), generator=g, dtype=torch.uint8)
    clip[1, 0] = frame.view(H, W, 3)
    clip[2, 0, :, :, 1] = 77
    return clip
