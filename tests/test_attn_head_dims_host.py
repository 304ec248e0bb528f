"""Head dims of vtx_attn_fwd / vtx_attn_bwd and the attn_hd switch, as far as a host without a GPU can tell (argument
validation happens before any launch: tests/test_abi.py, test_bad_arguments_are_rejected_without_a_gpu).

  * head_dim 32, 64, 96 and 128 pass the head-dim check of csrc/attn.hip's make_params: with a null qkv it is the pointer /
    alignment check behind it that refuses the call;
  * every other head dim is refused by the head-dim check itself;
  * attn_hd = mfma | valu (bf16 attention of more than 32 tokens at head_dim 32 / 96 / 128: the MFMA kernels of
    csrc/attn_hd.hip, the default, or the VALU kernels of csrc/attn.hip); anything else is refused; VTX_ATTN_HD seeds it.
"""
import ctypes
import os
import re
import subprocess
import sys

import pytest

from helpers import ROOT

PKG = os.path.join(ROOT, 'videotransformer-pytorch_amd')
SUPPORTED = (32, 64, 96, 128)
EINVAL, EALIGN = -1, -2


@pytest.fixture
def attn_hd():
    """set(value) -> vtx.set_option('attn_hd', value); back to the default afterwards (tests/conftest.py's vtx_opts does
    not know this switch)."""
    import vtx
    try:
        yield lambda v: vtx.set_option('attn_hd', v)
    finally:
        vtx.set_option('attn_hd', 'mfma')


def _descs(hd, dtype):
    from vtx import _lib
    a = _lib.AttnDesc()
    a.dtype, a.mode = dtype, _lib.ATTN_CONTIG
    a.S, a.L, a.H, a.hd = 1, 40, 2, hd
    a.ld_qkv, a.ld_out, a.scale = 3 * 2 * hd, 2 * hd, 0.125
    b = _lib.AttnBwdDesc()
    b.f = a
    return a, b


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
@pytest.mark.parametrize('hd', SUPPORTED)
def test_supported_head_dims_reach_the_pointer_check(hd, dtype):
    from vtx import _lib
    lib = _lib.load()
    a, b = _descs(hd, _lib.VTX_F32 if dtype == 'f32' else _lib.VTX_BF16)
    for fn, d in ((lib.vtx_attn_fwd, a), (lib.vtx_attn_bwd, b)):
        assert fn(ctypes.byref(d), None) == EALIGN
        msg = lib.vtx_last_error_string()
        assert b'qkv alignment' in msg and b'head_dim' not in msg and str(hd).encode() not in msg, msg


@pytest.mark.parametrize('hd', [0, 16, 48, 80, 256])
def test_other_head_dims_are_refused_by_the_head_dim_check(hd):
    from vtx import _lib
    lib = _lib.load()
    a, b = _descs(hd, _lib.VTX_BF16)
    for fn, d in ((lib.vtx_attn_fwd, a), (lib.vtx_attn_bwd, b)):
        assert fn(ctypes.byref(d), None) == EINVAL
        msg = lib.vtx_last_error_string()
        assert f'head_dim {hd} unsupported'.encode() in msg, msg


def test_attn_hd_option_is_accepted(attn_hd):
    import vtx
    attn_hd('valu')
    attn_hd('mfma')
    for value in ('x', '', '0', '1', 'MFMA', 'mfma ', 'vALU', 'auto'):
        with pytest.raises(vtx.VtxError):
            vtx.set_option('attn_hd', value)
    for name in ('attn_h', 'attn_hd_', 'ATTN_HD', 'attnhd'):
        with pytest.raises(vtx.VtxError):
            vtx.set_option(name, 'mfma')
    vtx.set_option('attn_f32', 'valu')               # the sibling it is modelled on keeps working beside it
    vtx.set_option('attn_f32', 'mfma')


_CHILD = r'''
import sys
sys.path.insert(0, sys.argv[1])
import vtx
from vtx import _lib
_lib.load()
for v in ('valu', 'mfma'):
    vtx.set_option('attn_hd', v)
try:
    vtx.set_option('attn_hd', 'x')
    print('accepted x')
except vtx.VtxError:
    print('refused x')
print('loaded')
'''


@pytest.mark.parametrize('env', [None, 'valu', 'mfma', 'x'])
def test_attn_hd_environment_seed_loads_and_parses(env):
    """An unparsable VTX_ATTN_HD keeps the default, like the other switches (csrc/api.hip: options())."""
    import __graft_entry__ as ge
    ge.ensure_built()
    e = dict(os.environ)
    e.pop('VTX_ATTN_HD', None)
    if env is not None:
        e['VTX_ATTN_HD'] = env
    r = subprocess.run([sys.executable, '-c', _CHILD, PKG], env=e, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert 'refused x' in r.stdout and 'accepted x' not in r.stdout and 'loaded' in r.stdout


def test_header_library_and_docs_name_the_option():
    hdr = open(os.path.join(ROOT, 'include', 'vtx.h')).read()
    assert '"attn_hd" = mfma|valu' in hdr
    api = open(os.path.join(PKG, 'csrc', 'api.hip')).read()
    assert '{"VTX_ATTN_HD", "attn_hd"}' in api
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    assert re.search(r'^\| `attn_hd` \| `VTX_ATTN_HD` \|', doc, flags=re.M)
    build = open(os.path.join(PKG, 'csrc', 'build.py')).read()
    assert "'attn_hd.hip'" in build
