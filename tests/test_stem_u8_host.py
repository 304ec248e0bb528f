"""MaskFeat from uint8 clips, host side (no GPU): the C ABI of libvtx_stem.so (include/vtx_stem.h), the argument checks of its
two device entry points -- made before anything is launched, so they run here with never-dereferenced pointers --, the centre
frames vtx.hog_targets selects against video_transformer.center_frame_mask's keep table, and the refusal of CPU tensors."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

NAMES = ['vtx_hog_fwd_sel', 'vtx_im2col3d_u8', 'vtx_stem_last_error_string', 'vtx_stem_version']
EINVAL, EALIGN = -1, -2
I3 = ctypes.c_int * 3
F3 = ctypes.c_float * 3


def test_stem_library_header_and_binding_agree():
    """include/vtx_stem.h, vtx/_lib.py STEM_SIGNATURES and the export list of libvtx_stem.so name the same 4 symbols; none of them
    is declared in the other five headers or exported by libvtx.so (which keeps the HOG kernel's other entry point); the header
    compiles as C99."""
    import __graft_entry__ as ge
    from helpers import ROOT
    from vtx import _lib
    ge.ensure_built()

    def declared(header):
        src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', header)).read(), flags=re.S)
        return sorted(set(re.findall(r'\b(vtx_[a-z0-9_]+)\s*\(', src)))

    def exported(path):
        out = subprocess.run(['nm', '-D', '--defined-only', path], check=True, capture_output=True, text=True).stdout
        return sorted(ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith('vtx_'))
    names = declared('vtx_stem.h')
    assert names == sorted(_lib.STEM_SIGNATURES) and names == NAMES
    assert exported(_lib.STEM_LIB_PATH) == names
    for other in ('vtx.h', 'vtx_aug.h', 'vtx_randaug.h', 'vtx_views.h', 'vtx_mix.h'):
        assert not set(names) & set(declared(other))
    assert not set(names) & set(exported(_lib.LIB_PATH)) and 'vtx_hog_fwd' in exported(_lib.LIB_PATH)
    assert _lib.load_stem().vtx_stem_version() >= 100
    subprocess.run(['gcc', '-std=c99', '-fsyntax-only', '-x', 'c', os.path.join(ROOT, 'include', 'vtx_stem.h')], check=True)
    # the ctypes argument lists have the header's lengths
    assert len(_lib.STEM_SIGNATURES['vtx_im2col3d_u8'][1]) == 14 and len(_lib.STEM_SIGNATURES['vtx_hog_fwd_sel'][1]) == 10


def test_im2col3d_u8_rejects_bad_arguments_before_any_launch():
    """Null pointers, non-positive sizes, a bad dtype, a non-positive kernel or stride, a negative padding, a zero std, Kp too
    small or no multiple of 8, an empty output grid and the 2^31 index bounds: VTX_EINVAL (-1) with a reason, on a machine
    without a GPU -- nothing was launched.  rows off 16-byte alignment: VTX_EALIGN (-2); the clip may sit at any address."""
    from vtx import _lib
    lib = _lib.load_stem()
    err = lib.vtx_stem_last_error_string
    p = 4096                                                   # never dereferenced on the host
    mean, std = F3(0.45, 0.456, 0.406), F3(0.225, 0.224, 0.229)
    none3, nonei = ctypes.POINTER(ctypes.c_float)(), ctypes.POINTER(ctypes.c_int)()

    def call(dtype=1, B=2, T=4, H=32, W=32, k3=I3(3, 7, 7), s3=I3(2, 4, 4), p3=I3(1, 3, 3), Kp=448, clip=p, mean=mean, std=std, rows=2 * p):
        return lib.vtx_im2col3d_u8(dtype, B, T, H, W, k3, s3, p3, Kp, clip, mean, std, rows, None)
    for bad in (dict(clip=None), dict(rows=None), dict(mean=none3), dict(std=none3), dict(k3=nonei), dict(s3=nonei), dict(p3=nonei)):
        assert call(**bad) == EINVAL and b'null pointer' in err(), bad
    for bad in (dict(B=0), dict(T=0), dict(H=-32), dict(W=0)):
        assert call(**bad) == EINVAL and b'positive' in err(), bad
    assert call(dtype=2) == EINVAL and b'dtype' in err()
    for bad in (dict(k3=I3(0, 7, 7)), dict(s3=I3(2, 0, 4)), dict(p3=I3(1, 3, -1)), dict(k3=I3(3, 7, -7))):
        assert call(**bad) == EINVAL and b'axis' in err(), bad
    for i in range(3):
        z = F3(0.225, 0.224, 0.229)
        z[i] = 0.0
        assert call(std=z) == EINVAL and b'zero std' in err(), i
    assert call(Kp=440) == EINVAL and b'row width' in err()    # 3*3*7*7 = 441 > 440
    assert call(Kp=444) == EINVAL and b'row width' in err()    # covers 441, no multiple of 8
    assert call(Kp=0) == EINVAL and b'row width' in err()
    assert call(T=1, p3=I3(0, 3, 3)) == EINVAL and b'empty output grid' in err()     # 1 frame under a 3-frame kernel, no padding
    assert call(H=4, W=4, p3=I3(1, 0, 0)) == EINVAL and b'empty output grid' in err()
    assert call(B=64, T=16, H=1024, W=1024) == EINVAL and b'32-bit' in err()         # 3.2e9 clip bytes
    assert call(B=100, T=16, H=224, W=224, Kp=7168) == EINVAL and b'32-bit' in err()  # 2.4e8 clip bytes, but 2 508 800 rows x 896 stores
    for off in (2, 4, 8):
        assert call(rows=2 * p + off) == EALIGN and b'16-byte aligned' in err(), off
    assert call(rows=2 * p + 4, Kp=444) == EINVAL              # shape errors come first


def test_hog_fwd_sel_rejects_bad_arguments_before_any_launch():
    """Null pointers, a non-positive frame count, H or W no multiple of 16, an empty selection and a short table blob:
    VTX_EINVAL; frames / out off 16-byte, sel off 4-byte alignment: VTX_EALIGN.  vtx_hog_fwd of libvtx.so still refuses as before."""
    from vtx import _lib
    lib = _lib.load_stem()
    err = lib.vtx_stem_last_error_string
    p = 4096
    tb = _lib.load().vtx_hog_table_bytes()
    assert tb == 256 * 256 * 8 + 4096 * 4

    def call(frames=p, F=8, H=32, W=48, sel=2 * p, n=3, table=3 * p, table_bytes=tb, out=4 * p):
        return lib.vtx_hog_fwd_sel(frames, F, H, W, sel, n, table, table_bytes, out, None)
    for bad in (dict(frames=None), dict(sel=None), dict(table=None), dict(out=None)):
        assert call(**bad) == EINVAL and b'null pointer' in err(), bad
    for bad in (dict(F=0), dict(F=-1), dict(H=40), dict(W=40), dict(H=0), dict(W=2048)):
        assert call(**bad) == EINVAL and b'multiples of 16' in err(), bad
    for n in (0, -3):
        assert call(n=n) == EINVAL and b'empty selection' in err(), n
    assert call(table_bytes=256 * 256 * 8) == EINVAL and b'table blob' in err()      # the magnitudes alone
    assert call(frames=p + 8) == EALIGN and b'16-byte aligned' in err()
    assert call(out=4 * p + 8) == EALIGN and b'16-byte aligned' in err()
    assert call(sel=2 * p + 2) == EALIGN and b'4-byte aligned' in err()
    assert call(sel=2 * p + 2, n=0) == EINVAL                  # shape errors come first
    assert _lib.load().vtx_hog_fwd(None, 1, 224, 224, None, 0, None, None, None) == EINVAL


MARKERS = [[[0, 1]], [[1, 2], [3, 1]], [], [[0, 4]], [[2, 2], [0, 2], [2, 2]], [[7, 1]], [[0, 3], [3, 5]]]


@pytest.mark.parametrize('tstride', [1, 2, 4])
def test_center_frames_match_center_frame_mask(tstride):
    """ops.hog_center_frames (what hog_targets uploads) selects exactly the frames center_frame_mask keeps: same expression
    start*ts + span*ts//2, duplicates once, a clip without markers none, sorted flat indices b*T + centre."""
    from video_transformer import center_frame_mask
    from vtx import ops
    T = 8 * tstride
    mask = torch.ones(len(MARKERS), 8, 2, 2, dtype=torch.int32)
    _, keep = center_frame_mask(mask, MARKERS, T, tstride)
    sel = ops.hog_center_frames(MARKERS, T, tstride)
    assert sel == sorted(set(sel)) and all(isinstance(i, int) for i in sel)
    assert sel == keep.reshape(-1).nonzero().reshape(-1).tolist()
    assert not any(T * 2 <= i < T * 3 for i in sel)            # the clip with the empty marker list
    assert ops.hog_center_frames([[] for _ in range(3)], T, tstride) == []


def test_center_frame_outside_the_clip_raises():
    from vtx import ops
    assert ops.hog_center_frames([[[3, 1]]], 8, 2) == [7]
    for markers, T in (([[[4, 0]]], 8), ([[[3, 2]]], 8), ([[], [[-1, 1]]], 8), ([[[0, 1]]], 1)):
        with pytest.raises(ValueError, match='centre frame'):
            ops.hog_center_frames(markers, T, 2)


def test_cpu_and_misshapen_uint8_clips_raise():
    """No host fallback: ops.im2col3d_u8, vtx.hog_targets, the stem module and MaskFeat refuse a CPU uint8 clip as every other
    entry does; the shape checks come first (reachable without a device) and raise ValueError."""
    import mvit
    import video_transformer as V
    import vtx
    from vtx import ops
    assert vtx.hog_targets is ops.hog_targets
    clip = torch.zeros(2, 4, 32, 32, 3, dtype=torch.uint8)
    k = ((3, 7, 7), (2, 4, 4), (1, 3, 3), 448, torch.float32)
    vtx.set_input_normalization((0.45, 0.456, 0.406), (0.225, 0.224, 0.229))
    try:
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            ops.im2col3d_u8(clip, *k)
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            vtx.hog_targets(clip, [[[0, 1]], []])
        stem = mvit.create_conv_patch_embed(in_channels=3, out_channels=16, conv_kernel_size=(3, 7, 7), conv_stride=(2, 4, 4),
                                            conv_padding=(1, 3, 3))
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            stem(clip)
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            V.MaskFeat(num_frames=4, img_size=32, backbone=torch.nn.Identity()).forward_features(clip)
        for bad in (clip.permute(0, 1, 4, 2, 3).contiguous(), clip[0], clip[..., :2]):
            with pytest.raises(ValueError, match=r'\[B,T,H,W,3\]'):
                ops.im2col3d_u8(bad, *k)
            with pytest.raises(ValueError, match=r'\[B,T,H,W,3\]'):
                vtx.hog_targets(bad, [[], []])
            if bad.ndim == 5:
                with pytest.raises(ValueError, match=r'\[B,T,H,W,3\]'):
                    stem(bad)
        with pytest.raises(TypeError, match='uint8'):
            ops.im2col3d_u8(clip.float(), *k)
        with pytest.raises(TypeError, match='uint8'):
            vtx.hog_targets(clip.float(), [[], []])
    finally:
        vtx.set_input_normalization(None, None)
