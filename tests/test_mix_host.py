"""Mixup / CutMix on uint8 clips, host side (no GPU): the C ABI of libvtx_mix.so (include/vtx_mix.h), the argument checks of
its two device entry points -- made before anything is launched, so they run here with never-dereferenced pointers -- and
the checks of the vtx.MixedClip carrier."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

NAMES = ['vtx_cutmix_batch_u8', 'vtx_mix_last_error_string', 'vtx_mix_version', 'vtx_patch_rows_mix_u8']
EINVAL, EALIGN = -1, -2


def test_mix_library_header_and_binding_agree():
    """include/vtx_mix.h, vtx/_lib.py MIX_SIGNATURES and the export list of libvtx_mix.so name the same 4 symbols; none of them is
    declared in the other four headers; the header compiles as C99."""
    import __graft_entry__ as ge
    from helpers import ROOT
    from vtx import _lib
    ge.ensure_built()

    def declared(header):
        src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', header)).read(), flags=re.S)
        return sorted(set(re.findall(r'\b(vtx_[a-z0-9_]+)\s*\(', src)))
    names = declared('vtx_mix.h')
    assert names == sorted(_lib.MIX_SIGNATURES) and names == NAMES
    out = subprocess.run(['nm', '-D', '--defined-only', _lib.MIX_LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert sorted(ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith('vtx_')) == names
    for other in ('vtx.h', 'vtx_aug.h', 'vtx_randaug.h', 'vtx_views.h'):
        assert not set(names) & set(declared(other))
    assert _lib.load_mix().vtx_mix_version() >= 100
    subprocess.run(['gcc', '-std=c99', '-fsyntax-only', '-x', 'c', os.path.join(ROOT, 'include', 'vtx_mix.h')], check=True)


def test_cutmix_u8_rejects_bad_arguments_before_any_launch():
    """A null pointer, non-positive sizes, an odd batch, a box outside the frame or turned inside out: VTX_EINVAL (-1) with a
    reason, on a machine without a GPU -- nothing was launched.  An empty box is VTX_OK and launches nothing either; no
    alignment is asked of the pointer."""
    from vtx import _lib
    lib = _lib.load_mix()
    err = lib.vtx_mix_last_error_string
    p = 4096                                                   # never dereferenced on the host

    def call(B=4, T=2, H=10, W=7, clip=p, box=(2, 9, 1, 6)):
        return lib.vtx_cutmix_batch_u8(B, T, H, W, clip, *box, None)
    assert call(clip=None) == EINVAL and b'null pointer' in err()
    for bad in (dict(B=0), dict(B=-2), dict(T=0), dict(H=0), dict(W=-7)):
        assert call(**bad) == EINVAL and b'positive' in err(), bad
    assert call(B=3) == EINVAL and b'even' in err()
    assert call(B=1) == EINVAL and b'even' in err()
    for box in ((-1, 9, 1, 6), (2, 11, 1, 6), (2, 9, -1, 6), (2, 9, 1, 8), (9, 2, 1, 6), (2, 9, 6, 1)):
        assert call(box=box) == EINVAL and b'outside' in err(), box
    for box in ((3, 3, 1, 6), (2, 9, 4, 4), (0, 0, 0, 0), (10, 10, 7, 7)):
        assert call(box=box) == 0, box                         # empty: VTX_OK, and no launch (there is no device here)
        assert call(box=box, clip=p + 1) == 0, box
    assert call(clip=p + 1, B=3) == EINVAL                     # an unaligned pointer is no error of its own


def test_patch_rows_mix_u8_rejects_bad_arguments_before_any_launch():
    """Null pointers, non-positive sizes, an odd batch, ps not a multiple of 4, H or W not a multiple of ps, T not a multiple of
    ts, a zero std, a bad dtype and a short ldr: VTX_EINVAL with a reason; a clip that is not 4-byte aligned: VTX_EALIGN (-2)."""
    from vtx import _lib
    lib = _lib.load_mix()
    err = lib.vtx_mix_last_error_string
    p = 4096
    f3 = ctypes.c_float * 3
    mean, std = f3(0.45, 0.456, 0.406), f3(0.225, 0.224, 0.229)
    none3 = ctypes.POINTER(ctypes.c_float)()

    def call(dtype=0, B=2, T=4, H=32, W=48, ps=16, ts=2, clip=p, mean=mean, std=std, rows=2 * p, ldr=None):
        ldr = 3 * ts * ps * ps if ldr is None else ldr
        return lib.vtx_patch_rows_mix_u8(dtype, B, T, H, W, ps, ts, clip, mean, std, 0.3, 0.7, rows, ldr, 1, None)
    for bad in (dict(clip=None), dict(rows=None), dict(mean=none3), dict(std=none3)):
        assert call(**bad) == EINVAL and b'null pointer' in err(), bad
    for bad in (dict(B=0), dict(T=0), dict(H=-32), dict(W=0), dict(ps=0), dict(ts=0), dict(ps=-16)):
        assert call(**bad) == EINVAL and b'positive' in err(), bad
    assert call(B=3) == EINVAL and b'even' in err()
    assert call(ps=6, H=36, W=48, ldr=4096) == EINVAL and b'multiple' in err()          # ps % 4
    assert call(H=40) == EINVAL and b'multiple' in err()                                # H % ps
    assert call(W=40) == EINVAL and b'multiple' in err()                                # W % ps
    assert call(T=3) == EINVAL and b'multiple' in err()                                 # T % ts
    for i in range(3):
        z = f3(0.225, 0.224, 0.229)
        z[i] = 0.0
        assert call(std=z) == EINVAL and b'zero std' in err(), i
    assert call(dtype=2) == EINVAL and b'dtype' in err()
    assert call(ldr=3 * 2 * 256 - 1) == EINVAL and b'ldr' in err()
    for off in (1, 2, 3):
        assert call(clip=p + off) == EALIGN and b'4-byte aligned' in err(), off
    assert call(clip=p + 2, B=3) == EINVAL                     # shape errors come first


def test_mixed_clip_checks_its_clip():
    """vtx.MixedClip is the plain carrier of (uint8 clip, lam): other dtypes, a last dimension that is not 3, an odd batch and CPU
    tensors are refused (the shape checks come first, so they are reachable without a device)."""
    import vtx
    from vtx import ops
    assert vtx.MixedClip is ops.MixedClip and not issubclass(ops.MixedClip, torch.Tensor)
    ok = torch.zeros(2, 4, 8, 12, 3, dtype=torch.uint8)
    with pytest.raises(TypeError, match='uint8'):
        ops.MixedClip(ok.float(), 0.3)
    with pytest.raises(TypeError, match='uint8'):
        ops.MixedClip(ok.to(torch.int8), 0.3)
    with pytest.raises(TypeError, match='uint8'):
        ops.MixedClip(ok.numpy(), 0.3)
    with pytest.raises(ValueError, match=r'\[B,T,H,W,3\]'):
        ops.MixedClip(torch.zeros(2, 4, 3, 8, 12, dtype=torch.uint8), 0.3)
    with pytest.raises(ValueError, match=r'\[B,T,H,W,3\]'):
        ops.MixedClip(ok[0], 0.3)
    with pytest.raises(ValueError, match='even'):
        ops.MixedClip(torch.zeros(3, 4, 8, 12, 3, dtype=torch.uint8), 0.3)
    with pytest.raises(ValueError, match='contiguous'):
        ops.MixedClip(torch.zeros(2, 4, 8, 12, 6, dtype=torch.uint8)[..., ::2], 0.3)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.MixedClip(ok, 0.3)


def test_cpu_uint8_batches_raise():
    """No host fallback: Mixup on a CPU uint8 batch and cutmix_batch_u8_ on a CPU clip raise, as the float forms do."""
    from mixup import Mixup
    from vtx import ops
    clip = torch.zeros(2, 4, 8, 12, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.cutmix_batch_u8_(clip, 0, 4, 0, 4)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        Mixup(num_classes=5)(clip, torch.zeros(2, dtype=torch.long))
