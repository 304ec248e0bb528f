"""The packed MFMA attention kernels for up to 32 tokens at head_dim 32, 96 and 128 (csrc/attn_hd.hip, namespace hdsmall), as
far as a host without a GPU can tell:

  * the object csrc/build.py compiles from attn_hd.hip exists after a build and holds the host stub of a forward and of a
    backward kernel per head dim, in both layouts (CONTIG, TIME_CLS) and both workgroup shapes (attn_hw_* = 0 / n);
  * csrc/attn.hip routes to them under the attn_hd switch, and csrc/build.py, include/vtx.h and INTEGRATION.md say what
    the switch now covers.
"""
import os
import re
import subprocess

from helpers import ROOT

PKG = os.path.join(ROOT, 'videotransformer-pytorch_amd')
OBJ = os.path.join(PKG, 'csrc', '_obj', 'attn_hd.o')


def _stubs():
    import __graft_entry__ as ge
    ge.ensure_built()
    assert os.path.isfile(OBJ), 'csrc/_obj/attn_hd.o is missing after a build'
    out = subprocess.run(['nm', '-C', '--defined-only', OBJ], check=True, capture_output=True, text=True).stdout
    return re.findall(r'vtx::hdsmall::__device_stub__(fwd|bwd)_kernel<(\d+), (true|false), (true|false)>', out)


def test_object_holds_a_forward_and_a_backward_kernel_per_head_dim():
    stubs = set(_stubs())
    want = {(k, str(hd), hw, cls) for k in ('fwd', 'bwd') for hd in (32, 96, 128) for hw in ('true', 'false') for cls in ('true', 'false')}
    assert stubs == want, f'missing {sorted(want - stubs)}, unexpected {sorted(stubs - want)}'


def test_library_still_exports_what_the_header_declares():
    """No new export: the kernels sit behind vtx_attn_fwd / vtx_attn_bwd."""
    import __graft_entry__ as ge
    ge.ensure_built()
    out = subprocess.run(['nm', '-D', '--defined-only', os.path.join(PKG, 'libvtx.so')], check=True, capture_output=True, text=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert {'vtx_attn_fwd', 'vtx_attn_bwd'} <= names
    assert not [n for n in names if 'hd_small' in n and n.startswith('vtx_')]


def test_sources_and_docs_name_the_route():
    read = lambda *p: open(os.path.join(*p)).read()          # noqa: E731
    build = read(PKG, 'csrc', 'build.py')
    assert "'attn_hd.hip'" in build
    route = read(PKG, 'csrc', 'attn.hip')
    assert re.search(r'options\(\)\.attn_hd && attn_hd_small_eligible\(dtype, mode, L, hd\)', route)
    assert route.index('options().attn_valu') < route.index('attn_hd_small_eligible')          # attn_valu=1 still wins
    kernels = read(PKG, 'csrc', 'attn_hd.hip')
    assert 'namespace hdsmall' in kernels and 'attn_fwd_hd_small_launch' in kernels and 'attn_bwd_hd_small_launch' in kernels
    hdr = read(ROOT, 'include', 'vtx.h')
    assert '"attn_hd" = mfma|valu' in hdr
    i = hdr.index('"attn_hd" = mfma|valu')
    assert 'up to 32 tokens' in hdr[i:i + 900], 'include/vtx.h: the attn_hd comment does not name the packed route'
    doc = read(ROOT, 'INTEGRATION.md')
    row = re.search(r'^\| `attn_hd` \| `VTX_ATTN_HD` \|.*$', doc, flags=re.M)
    assert row and 'up to 32 tokens' in row.group(0) and 'TIME_CLS' in row.group(0)
