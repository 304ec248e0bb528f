"""Host-side checks of the space-then-time operator order (no GPU): the two attention layouts validate their shape fields
before anything is launched, and a space-then-time block has the reference's state_dict keys."""
import ctypes

import pytest


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as ge
    ge.ensure_built()
    from vtx import _lib
    L = _lib.load()
    L.vtx_last_error_string.restype = ctypes.c_char_p
    return _lib, L


def _desc(_lib, mode, S, L, B, T, P):
    d = _lib.AttnDesc()
    d.dtype, d.mode = _lib.VTX_BF16, mode
    d.S, d.L, d.H, d.hd = S, L, 2, 64
    d.B, d.T, d.P = B, T, P
    d.ld_qkv, d.ld_out, d.scale = 3 * 128, 128, 0.125
    return d


BAD = [('TIME_CLS', 'ATTN_TIME_CLS', dict(S=2 * 5, L=8, B=2, T=8, P=5)),        # L != T + 1
       ('TIME_CLS', 'ATTN_TIME_CLS', dict(S=2 * 8, L=9, B=2, T=8, P=5)),        # S != B * P
       ('TIME_CLS', 'ATTN_TIME_CLS', dict(S=10, L=9, B=0, T=8, P=5)),           # B missing
       ('SPACE_NOCLS', 'ATTN_SPACE_NOCLS', dict(S=2 * 8, L=6, B=2, T=8, P=5)),  # L != P (the cls layout's length)
       ('SPACE_NOCLS', 'ATTN_SPACE_NOCLS', dict(S=2 * 5, L=5, B=2, T=8, P=5)),  # S != B * T
       ('SPACE_NOCLS', 'ATTN_SPACE_NOCLS', dict(S=16, L=5, B=2, T=8, P=0))]     # P missing


@pytest.mark.parametrize('name,const,kw', BAD)
def test_inconsistent_shapes_are_rejected_by_name(lib, name, const, kw):
    _lib, L = lib
    d = _desc(_lib, getattr(_lib, const), **kw)
    assert L.vtx_attn_fwd(ctypes.byref(d), None) == -1
    msg = L.vtx_last_error_string().decode()
    assert name in msg and 'bad mode' not in msg, msg
    b = _lib.AttnBwdDesc()
    b.f = d
    assert L.vtx_attn_bwd(ctypes.byref(b), None) == -1
    assert name in L.vtx_last_error_string().decode()


def test_consistent_shapes_pass_the_shape_checks(lib):
    """... and stop at the next one (a null qkv pointer), so nothing is launched."""
    _lib, L = lib
    for const, kw in (('ATTN_TIME_CLS', dict(S=10, L=9, B=2, T=8, P=5)), ('ATTN_SPACE_NOCLS', dict(S=16, L=5, B=2, T=8, P=5))):
        d = _desc(_lib, getattr(_lib, const), **kw)
        assert L.vtx_attn_fwd(ctypes.byref(d), None) != 0
        assert 'qkv alignment' in L.vtx_last_error_string().decode()


def test_unknown_mode_is_still_rejected(lib):
    _lib, L = lib
    d = _desc(_lib, 4, S=10, L=9, B=2, T=8, P=5)
    assert L.vtx_attn_fwd(ctypes.byref(d), None) == -1
    assert 'bad mode' in L.vtx_last_error_string().decode()


def test_state_dict_keys_of_a_space_then_time_block():
    """The keys of the reference's BasicTransformerBlock(operator_order=['space_attn', 'time_attn', 'ffn']): the spatial block
    first, no temporal_fc in the temporal block (it attends over the cls token; reference transformer.py:207-209)."""
    import transformer as T_
    blk = T_.BasicTransformerBlock(128, 2, 8, 256, ['space_attn', 'time_attn', 'ffn'])
    assert blk.attentions[0].use_cls_token is False and blk.attentions[1].use_cls_token is True
    assert type(blk.attentions[0]) is T_.DividedSpatialAttentionWithPreNorm
    sub = ['norm.weight', 'norm.bias', 'attn.qkv.weight', 'attn.qkv.bias', 'attn.proj.weight', 'attn.proj.bias']
    want = [f'attentions.{i}.{k}' for i in (0, 1) for k in sub]
    want += [f'ffns.0.{k}' for k in ('norm.weight', 'norm.bias', 'layers.0.0.weight', 'layers.0.0.bias', 'layers.1.weight', 'layers.1.bias')]
    assert list(blk.state_dict().keys()) == want
