"""Dropout on the HIP path, what can be checked without a GPU: the NumPy restatement of the mask contract (tests/dropout_ref.py)
against the published Philox4x32-10 known answers, ops.dropout_params, the C ABI of libvtx_dropout.so (include/vtx_dropout.h) and
the argument checks of vtx_dropout_rows, and the construction of the modules that used to refuse a dropout probability."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import dropout_ref as R
from model_common import SMALL

SEED = 0x9abcdef012345678


def _hex(words):
    return ' '.join(f'{int(w[0]):08x}' for w in words)


@pytest.mark.parametrize('counter,key,want', [
    ((0, 0, 0, 0), (0, 0), '6627e8d5 e169c58d bc57ac4c 9b00dbd8'),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, '408f276d 41c83b0e a20bc7c6 6d5451fd'),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), 'd16cfe09 94fdcceb 5001e420 24126ea1'),
])
def test_philox_known_answers(counter, key, want):
    assert _hex(R.philox4x32_10(counter, key)) == want


def test_dropout_params():
    from vtx import ops
    assert ops.dropout_params(0) == (0, 1.0)
    assert ops.dropout_params(0.5) == (2 ** 31, 2.0)
    assert ops.dropout_params(1) == (2 ** 32, 0.0)
    thr, scale = ops.dropout_params(0.1)
    assert scale == float(np.float32(1) / np.float32(0.9))
    assert thr == R.threshold(0.1) == int(0.1 * 2 ** 32)
    for p in (-0.1, 1.5):
        with pytest.raises(ValueError):
            ops.dropout_params(p)
    for p in (0, 0.1, 0.25, 0.5, 1):                     # the helper restates the same two numbers
        assert ops.dropout_params(p) == (R.threshold(p), float(R.keep_scale(p)))


@pytest.mark.parametrize('rows,D,p,want', [(6, 40, 0.25, 0.7625), (64, 768, 0.1, 0.89935)])
def test_keep_fraction_of_the_restatement(rows, D, p, want):
    """A sanity check on the helper, not on the kernel: the keep fraction lies within 4 sigma of the binomial mean (computed
    when the test was written: 0.7625 and 0.89935, both within 0.5 sigma)."""
    keep = R.keep_mask(SEED, 0, 0, rows, D, p)
    n = rows * D
    frac = keep.sum() / n
    print(f'{rows}x{D} p={p}: kept {frac:.5f}')
    assert abs(frac - want) < 5e-6
    assert abs(frac - (1 - p)) <= 4 * np.sqrt(p * (1 - p) / n)


def test_sites_and_offsets_of_the_restatement():
    a = R.words(SEED, 0, 0, 7, 40)
    assert not np.array_equal(a, R.words(SEED, 1, 0, 7, 40))
    # e0 shifts the element index: the launch at e0 = 3 rows continues the launch at e0 = 0
    assert np.array_equal(R.words(SEED, 0, 3 * 40, 4, 40), a[3:])
    assert not np.array_equal(R.words(SEED, 0, 2 ** 34, 7, 40), a)


def test_apply_rounds_once():
    rs = np.random.RandomState(0)
    x = R.bf16_round(rs.randn(6, 40).astype(np.float32))
    y = R.apply(x, SEED, 0, 0.5, bf16=True)
    keep = R.keep_mask(SEED, 0, 0, 6, 40, 0.5)
    assert np.array_equal(y[keep], x[keep] * 2) and not y[~keep].any()
    assert np.array_equal(R.apply(x, SEED, 0, 0.0), x)
    assert not R.apply(x, SEED, 0, 1.0).any()


def test_dropout_library_header_and_binding_agree():
    """include/vtx_dropout.h, vtx/_lib.py DROPOUT_SIGNATURES and the export list of libvtx_dropout.so name the same 3 symbols; none
    of them is declared in the other seven headers; the header compiles as C99."""
    import __graft_entry__ as ge
    from helpers import ROOT
    from vtx import _lib
    ge.ensure_built()

    def declared(header):
        src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', header)).read(), flags=re.S)
        return sorted(set(re.findall(r'\b(vtx_[a-z0-9_]+)\s*\(', src)))
    names = declared('vtx_dropout.h')
    assert names == sorted(_lib.DROPOUT_SIGNATURES) and names == ['vtx_dropout_last_error_string', 'vtx_dropout_rows', 'vtx_dropout_version']
    out = subprocess.run(['nm', '-D', '--defined-only', _lib.DROPOUT_LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert sorted(ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith('vtx_')) == names
    for other in ('vtx.h', 'vtx_aug.h', 'vtx_randaug.h', 'vtx_views.h', 'vtx_mix.h', 'vtx_stem.h', 'vtx_ragged.h'):
        assert not set(names) & set(declared(other))
    assert _lib.load_dropout().vtx_dropout_version() >= 100
    subprocess.run(['gcc', '-std=c99', '-fsyntax-only', '-x', 'c', os.path.join(ROOT, 'include', 'vtx_dropout.h')], check=True)


def test_bad_arguments_are_rejected_without_a_gpu():
    from vtx import _lib
    lib = _lib.load_dropout()
    ident = _lib.IDENT
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.cast(buf, ctypes.c_void_p).value
    p += (-p) % 16

    def run(x=p, y=p, rows=2, D=16, e0=0):
        return lib.vtx_dropout_rows(_lib.VTX_F32, rows, D, x, D, ident, y, D, ident, None, D, ident, None, 0, None, 1, 0, 1, 0,
                                    2 ** 31, 2.0, SEED, 0, e0, None)
    for kw, word in ((dict(x=None), b'null'), (dict(y=None), b'null'), (dict(D=12), b'multiple of 8'), (dict(e0=2), b'multiple of 4'),
                     (dict(rows=0), b'positive')):
        assert run(**kw) == -1, kw
        msg = lib.vtx_dropout_last_error_string()
        assert b'dropout_rows' in msg and word in msg, (kw, msg)


def test_modules_construct_with_dropout():
    import transformer as T
    import video_transformer as V
    m = V.TimeSformer(num_frames=2, dropout_p=0.1, **SMALL)
    assert m.drop_after_pos.p == 0.1 and m.drop_after_time.p == 0.1
    v = V.ViViT(num_frames=4, dropout_p=0.1, **SMALL)
    assert v.drop_after_time.p == 0.1
    f = T.FFNWithPreNorm(embed_dims=128, hidden_channels=256, dropout_p=0.1)
    assert f.dropout_p == 0.1 and f.layers[1].__class__ is torch.nn.Linear
    a = T.Attention(128, num_heads=2, attn_drop=0.1)
    assert a.attn_drop.p == 0.1
    with pytest.raises(ValueError):
        V.TimeSformer(num_frames=2, dropout_p=1.5, **SMALL)
