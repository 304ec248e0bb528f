"""The attn_long switch of vtx_set_option (bf16 attention of more than 256 tokens: 1 = the MFMA kernels of
csrc/attn_long.hip, 0 = the VALU kernels) -- no GPU needed.  Parsed like its 0|1 siblings (attn_valu: atoi(value) != 0),
added without a new exported symbol."""
import ctypes
import os
import re
import subprocess

import pytest

from helpers import ROOT


@pytest.fixture
def attn_long():
    """set(value) -> vtx.set_option('attn_long', value); back to the default afterwards (tests/conftest.py's vtx_opts does
    not know this switch)."""
    import vtx
    try:
        yield lambda v: vtx.set_option('attn_long', v)
    finally:
        vtx.set_option('attn_long', '1')


def test_attn_long_option_is_accepted(attn_long):
    import vtx
    attn_long('0')
    attn_long('1')
    vtx.set_option('attn_valu', '1')                 # the sibling keeps working beside it
    vtx.set_option('attn_valu', '0')
    for name in ('attn_lon', 'attn_long_', 'ATTN_LONG', 'attnlong'):
        with pytest.raises(vtx.VtxError):
            vtx.set_option(name, '1')


def test_attn_long_values_parse_like_attn_valu(attn_long):
    """The 0|1 switches take atoi(value) != 0: whatever attn_valu accepts, attn_long accepts, and the other way round."""
    import vtx
    try:
        for value in ('0', '1', '2', '-1', ' 1', 'on', ''):
            outcome = []
            for name in ('attn_valu', 'attn_long'):
                try:
                    vtx.set_option(name, value)
                    outcome.append('ok')
                except vtx.VtxError:
                    outcome.append('rejected')
            assert outcome[0] == outcome[1], (value, outcome)
    finally:
        vtx.set_option('attn_valu', '0')


def test_no_new_exported_symbol():
    """The library's export list is the header's 62 declarations: the long-sequence kernels sit behind vtx_attn_fwd / _bwd."""
    import __graft_entry__ as ge
    ge.ensure_built()
    src = open(os.path.join(ROOT, 'include', 'vtx.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    declared = sorted(set(re.findall(r'\b(vtx_[a-z0-9_]+)\s*\(', src)))
    assert len(declared) == 62
    lib = os.path.join(ROOT, 'videotransformer-pytorch_amd', 'libvtx.so')
    out = subprocess.run(['nm', '-D', '--defined-only', lib], check=True, capture_output=True, text=True).stdout
    exported = sorted(ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith('vtx_'))
    assert exported == declared
    assert hasattr(ctypes.CDLL(lib), 'vtx_set_option')


def test_long_kernels_have_no_scratch_and_no_scalar_memory_writes():
    """tools/check_isa.py over the compiled csrc/attn_long.hip: three kernels, no scratch traffic, no scalar-unit writes."""
    import sys
    import __graft_entry__ as ge
    ge.ensure_built()
    obj = os.path.join(ROOT, 'videotransformer-pytorch_amd', 'csrc', '_obj', 'attn_long.o')
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import check_isa
    if not os.path.exists(obj) or not os.path.exists(check_isa.OBJDUMP):
        pytest.skip('needs the compiled object of csrc/attn_long.hip and llvm-objdump')
    assert check_isa.check_plain(obj, ['attn_fwd_long_kernel', 'attn_bwd_dq_long_kernel', 'attn_bwd_dkv_long_kernel']) == []
