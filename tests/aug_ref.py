"""CPU restatements for the clip-augmentation tests (tests/test_aug_host.py, tests/test_gpu_aug.py).  No tests here.

Two independent expectations for the resampler:
  * ``torch_resized_crop``: what torchvision's resized_crop (+ hflip) computes on a tensor -- crop, torch.nn.functional.interpolate
    (align_corners=False) of the float image, clamp, round, uint8 -- in plain torch;
  * ``table_eval``: a float64 evaluation  Wy . img . Wx^T  of the tables the library builds (vtx_resample_build_table).
A third, ``resample_f32``, restates the kernels' own float32 operation order and their clamp of the tap windows: the exact
bytes for any table, ``edge_table``'s bent ones included.
And ``jitter_ref``: torchvision's ColorJitter arithmetic (brightness / contrast / saturation blends) on a uint8 [T,H,W,3] clip.
"""
import numpy as np
import torch
import torch.nn.functional as F

SRC_HW = (40, 56)
OUT_HW = (32, 32)
#: (top, left, height, width): a downscale (more than 4 taps under antialias), an upscale whose taps fold on every border, the identity
BOXES = [(0, 0, 40, 56), (5, 7, 9, 12), (3, 4, 32, 32)]
MODES = [('bilinear', False), ('bilinear', True), ('bicubic', False), ('bicubic', True)]
TIE = 1e-3          # |float64 value - rounding tie| below which the float32 kernel may land on either side:
                    # 255 x ~24 taps x 2^-24 x a weight-magnitude sum <= 1.5 ~ 5e-4, doubled
TIE_SHARE = 0.03    # at most this share of the pixels of a case may be that close to a tie


def source_clip(B, T, hw, seed):
    """uint8 [B,T,H,W,3]: random frames; frame 0 of clip 0 all 0 and the last frame of clip 1 (of clip 0 when B = 1) all 255."""
    g = torch.Generator().manual_seed(seed)
    clip = torch.randint(0, 256, (B, T, hw[0], hw[1], 3), generator=g, dtype=torch.uint8)
    clip[0, 0] = 0
    if B * T > 1:
        clip[min(1, B - 1), T - 1] = 255
    return clip


def dense(table, src_len):
    """(first [n], count [n], weights [n, taps]) -> float64 [n, src_len]; asserts nothing: reads only the first count taps."""
    first, count, weights = table
    m = np.zeros((len(first), src_len), dtype=np.float64)
    for o in range(len(first)):
        for k in range(int(count[o])):
            m[o, int(first[o]) + k] += float(weights[o, k])
    return m


def table_eval(frames_u8, ytab, xtab):
    """frames uint8 [...,Hs,Ws,3] (NumPy or torch) -> float64 [...,H,W,3] = Wy . frame . Wx^T per channel, unrounded."""
    img = np.asarray(frames_u8, dtype=np.float64)
    wy, wx = dense(ytab, img.shape[-3]), dense(xtab, img.shape[-2])
    return np.einsum('ys,...sxc,wx->...ywc', wy, img, wx)


def near_tie(v64):
    """Where rint(clip(v64)) is decided by less than TIE."""
    v = np.clip(v64, 0.0, 255.0)
    return np.abs(np.abs(v - np.floor(v)) - 0.5) < TIE


def kernel_windows(table, src_len):
    """The tap windows as the kernels read them (clamp_taps, csrc/resample_band.h): count into 0 .. taps, first into 0 .. src_len,
    and a window that still runs past the source edge moved back to end at it -> (first [n], count [n])."""
    first, count, weights = (np.asarray(a) for a in table)
    c = np.clip(count.astype(np.int64), 0, weights.shape[1])
    f = np.clip(first.astype(np.int64), 0, src_len)
    over = f + c > src_len
    return np.where(over, np.maximum(src_len - c, 0), f), np.where(over, np.minimum(c, src_len), c)


def _pass_f32(img, table, axis):
    """out[o] = sum_k w[o, k] * img[first[o] + k] along ``axis``: taps in ascending order, every product and every sum rounded
    to float32 on its own (NumPy float32 arithmetic: no contraction).  Weights behind a count are not read."""
    img = np.moveaxis(img, axis, 0)
    f, c = kernel_windows(table, img.shape[0])
    w = np.asarray(table[2], dtype=np.float32)
    col = (-1,) + (1,) * (img.ndim - 1)
    out = np.zeros((len(f),) + img.shape[1:], dtype=np.float32)
    for k in range(int(c.max())):
        on = k < c
        wk = np.where(on, w[:, k], np.float32(0)).astype(np.float32)
        term = wk.reshape(col) * img[np.minimum(f + k, img.shape[0] - 1)]
        out = np.where(on.reshape(col), out + term, out)
    assert out.dtype == np.float32
    return np.moveaxis(out, 0, axis)


def resample_f32(frames_u8, ytab, xtab):
    """frames uint8 [...,Hs,Ws,3] -> uint8 [...,H,W,3]: the kernels' arithmetic restated operation for operation -- x pass, then
    y pass, float32, clamp to [0, 255], round half to even -- with their clamp of the tap windows.  Byte for byte."""
    img = np.asarray(frames_u8).astype(np.float32)
    out = _pass_f32(_pass_f32(img, xtab, -2), ytab, -3)
    return np.rint(np.clip(out, np.float32(0), np.float32(255))).astype(np.uint8)


def edge_table(src_len, out_len, mode='bicubic', antialias=True, max_taps=None, shift=0):
    """A table of vtx_resample_build_table (one spare weight column, NaN behind every count) bent at six outputs (out_len >= 13;
    ``shift`` 0 or 1 moves them by one) so that what the kernels do beyond a well-formed table shows:
      a window that starts right behind the last source sample, one that starts further behind, a negative first: the clamp acts;
      a count above the taps of the table (cut to them; that row's weights are all finite);
      a count of 0: the output row or column is 0 whatever the source holds."""
    from vtx import ops
    taps = max_taps or ops.resample_max_taps(src_len, out_len, mode, antialias) + 1
    f, c, w = ops.resample_table(src_len, 0, src_len, out_len, mode, antialias, max_taps=taps)
    assert out_len >= 13 and c.min() >= 1 and c.max() < taps
    for o in range(out_len):
        w[o, c[o]:] = np.nan
    f[1 + shift] = src_len
    f[4 + shift] = -3
    c[6 + shift] = 0
    w[8 + shift] = np.float32(1.0 / taps)
    c[8 + shift] = taps + 4
    f[out_len - 1 - shift] = src_len + 5
    assert (f + c > src_len).sum() >= 2 and (f < 0).any() and (c == 0).any() and (c > taps).any()
    return f, c, w


def torch_resize_float(frames_u8, box, out_hw, mode, antialias):
    """Crop, then F.interpolate of the float image: float32 [T,H,W,3], before the clamp and the rounding."""
    top, left, h, w = box
    x = frames_u8[:, top:top + h, left:left + w, :].permute(0, 3, 1, 2).float()
    y = F.interpolate(x, size=list(out_hw), mode=mode, align_corners=False, antialias=antialias)
    return y.permute(0, 2, 3, 1)


def torch_resized_crop(frames_u8, box, out_hw, mode, antialias, flip=False):
    """uint8 [T,Hs,Ws,3] -> uint8 [T,H,W,3]: resized_crop (clamp, round, cast) and the horizontal flip."""
    y = torch_resize_float(frames_u8, box, out_hw, mode, antialias).clamp(0, 255).round().to(torch.uint8)
    return y.flip(2) if flip else y


def _blend(img1, img2, ratio):
    ratio = float(ratio)
    return (ratio * img1 + (1.0 - ratio) * img2).clamp(0, 255).to(img1.dtype)


def _grey(img):
    r, g, b = img.unbind(dim=-3)
    return (0.2989 * r + 0.587 * g + 0.114 * b).to(img.dtype).unsqueeze(dim=-3)


def jitter_ref(frames_u8, jit_ops, factors, exact_mean=False):
    """uint8 [T,H,W,3]; ops in order (0 brightness, 1 contrast, 2 saturation), one factor each -> uint8 [T,H,W,3].
    exact_mean: the contrast mean is float32(the int64 sum of the greys) / float32(H W) instead of torch.mean of the float32 greys.
    The two agree while the sum stays below 2^24 (every frame of up to 65 793 pixels); beyond, torch.mean's value depends on its
    summation order (thread count, vector width) and the exact sum is what the device computes."""
    img = frames_u8.permute(0, 3, 1, 2).contiguous()
    for op, f in zip(jit_ops, factors):
        if op == 0:
            img = _blend(img, torch.zeros_like(img), f)
        elif op == 1:
            grey = _grey(img)
            if exact_mean:
                total = grey.to(torch.int64).sum(dim=(-3, -2, -1), keepdim=True)
                mean = total.to(torch.float32) / torch.tensor(float(grey[0].numel()), dtype=torch.float32)
            else:
                mean = torch.mean(grey.to(torch.float32), dim=(-3, -2, -1), keepdim=True)
            img = _blend(img, mean, f)
        elif op == 2:
            img = _blend(img, _grey(img), f)
        else:
            raise ValueError(op)
    return img.permute(0, 2, 3, 1).contiguous()
