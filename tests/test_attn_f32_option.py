"""The attn_f32 switch of vtx_set_option (fp32 attention of more than 32 tokens, head_dim 64: mfma = the exact-fp32 MFMA kernels
of csrc/attn_f32.hip, the default; valu = the VALU kernels of csrc/attn.hip) -- no GPU needed.  An enumerated option like
gemm_nt: two names, everything else is refused; VTX_ATTN_F32 seeds it once; no new exported symbol."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

from helpers import ROOT

PKG = os.path.join(ROOT, 'videotransformer-pytorch_amd')


@pytest.fixture
def attn_f32():
    """set(value) -> vtx.set_option('attn_f32', value); back to the default afterwards (tests/conftest.py's vtx_opts does
    not know this switch)."""
    import vtx
    try:
        yield lambda v: vtx.set_option('attn_f32', v)
    finally:
        vtx.set_option('attn_f32', 'mfma')


def test_attn_f32_option_is_accepted(attn_f32):
    import vtx
    attn_f32('valu')
    attn_f32('mfma')
    vtx.set_option('attn_valu', '1')                 # the siblings keep working beside it
    vtx.set_option('attn_valu', '0')
    vtx.set_option('attn_long', '0')
    vtx.set_option('attn_long', '1')
    for value in ('x', '', '0', '1', 'MFMA', 'mfma ', 'vALU', 'auto'):
        with pytest.raises(vtx.VtxError):
            vtx.set_option('attn_f32', value)
    for name in ('attn_f3', 'attn_f32_', 'ATTN_F32', 'attnf32'):
        with pytest.raises(vtx.VtxError):
            vtx.set_option(name, 'mfma')


# A rejected value leaves the option where it was, and VTX_ATTN_F32 seeds it: the library has no getter, so the child tells
# the state through what set_option / the environment accept -- an unparsable environment value keeps the default, like the
# other switches (csrc/api.hip: options()).
_CHILD = r'''
import sys
sys.path.insert(0, sys.argv[1])
import vtx
from vtx import _lib
_lib.load()
for v in ('valu', 'mfma'):
    vtx.set_option('attn_f32', v)
try:
    vtx.set_option('attn_f32', 'x')
    print('accepted x')
except vtx.VtxError:
    print('refused x')
print('version', _lib.load().vtx_version())
'''


@pytest.mark.parametrize('env', [None, 'valu', 'mfma', 'x'])
def test_attn_f32_environment_seed_loads_and_parses(env):
    import __graft_entry__ as ge
    ge.ensure_built()
    e = dict(os.environ)
    e.pop('VTX_ATTN_F32', None)
    if env is not None:
        e['VTX_ATTN_F32'] = env
    r = subprocess.run([sys.executable, '-c', _CHILD, PKG], env=e, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert 'refused x' in r.stdout and 'accepted x' not in r.stdout
    assert int(re.search(r'version (\d+)', r.stdout).group(1)) >= 230


def test_header_library_and_docs_name_the_option():
    hdr = open(os.path.join(ROOT, 'include', 'vtx.h')).read()
    assert '"attn_f32" = mfma|valu' in hdr
    api = open(os.path.join(PKG, 'csrc', 'api.hip')).read()
    assert '{"VTX_ATTN_F32", "attn_f32"}' in api
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    assert re.search(r'^\| `attn_f32` \| `VTX_ATTN_F32` \|', doc, flags=re.M)
    lib = open(os.path.join(PKG, 'vtx', '_lib.py')).read()
    assert 'vtx_set_option' in lib


def test_no_new_exported_symbol():
    """The library's export list is the header's 62 declarations: the fp32 MFMA kernels sit behind vtx_attn_fwd / _bwd."""
    import __graft_entry__ as ge
    ge.ensure_built()
    src = open(os.path.join(ROOT, 'include', 'vtx.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    declared = sorted(set(re.findall(r'\b(vtx_[a-z0-9_]+)\s*\(', src)))
    assert len(declared) == 62
    lib = os.path.join(PKG, 'libvtx.so')
    out = subprocess.run(['nm', '-D', '--defined-only', lib], check=True, capture_output=True, text=True).stdout
    exported = sorted(ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith('vtx_'))
    assert exported == declared
    assert hasattr(ctypes.CDLL(lib), 'vtx_set_option')


def test_f32_kernels_have_no_scratch_no_spills_and_the_fp32_mfma():
    """tools/check_isa.py over the compiled csrc/attn_f32.hip: three kernels, v_mfma_f32_32x32x2_f32 only, the MFMA count of one
    unrolled chunk, no scratch traffic, no spilled register, no scalar-unit writes."""
    import __graft_entry__ as ge
    ge.ensure_built()
    obj = os.path.join(PKG, 'csrc', '_obj', 'attn_f32.o')
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import check_isa
    if not os.path.exists(obj) or not os.path.exists(check_isa.OBJDUMP):
        pytest.skip('needs the compiled object of csrc/attn_f32.hip and llvm-objdump')
    assert check_isa.check_f32_attention(obj) == []
