"""The packed MFMA attention kernels for up to 32 tokens at head_dim 32, 64, 96 and 128 (the end of csrc/attn_hd.hip:
attn_fwd_small_kernel / attn_bwd_small_kernel<HD, HW, CLS>), as far as a host without a GPU can tell:

  * the object csrc/build.py compiles from attn_hd.hip exists after a build and holds the host stub of a forward and of a
    backward kernel per head dim, in both layouts (CONTIG, TIME_CLS) and both workgroup shapes (attn_hw_* = 0 / n), and
    the object of attn_mfma.hip, where head_dim 64 had a copy of its own, holds none;
  * csrc/attn.hip routes to them, head_dim 32, 96 and 128 under the attn_hd switch, and csrc/build.py, include/vtx.h and
    INTEGRATION.md say what the switch covers.
"""
import os
import re
import subprocess

from helpers import ROOT

PKG = os.path.join(ROOT, 'videotransformer-pytorch_amd')
OBJ = os.path.join(PKG, 'csrc', '_obj', 'attn_hd.o')
STUB = r'vtx::__device_stub__attn_(fwd|bwd)_small_kernel<(\d+), (true|false), (true|false)>'


def _stubs(obj=OBJ):
    import __graft_entry__ as ge
    ge.ensure_built()
    assert os.path.isfile(obj), f'csrc/_obj/{os.path.basename(obj)} is missing after a build'
    out = subprocess.run(['nm', '-C', '--defined-only', obj], check=True, capture_output=True, text=True).stdout
    return re.findall(STUB, out)


def test_object_holds_a_forward_and_a_backward_kernel_per_head_dim():
    stubs = set(_stubs())
    want = {(k, str(hd), hw, cls) for k in ('fwd', 'bwd') for hd in (32, 64, 96, 128) for hw in ('true', 'false') for cls in ('true', 'false')}
    assert len(want) == 32
    assert stubs == want, f'missing {sorted(want - stubs)}, unexpected {sorted(stubs - want)}'
    old = subprocess.run(['nm', '-C', '--defined-only', os.path.join(PKG, 'csrc', '_obj', 'attn_mfma.o')], check=True, capture_output=True,
                         text=True).stdout
    assert 'small_kernel' not in old, 'csrc/attn_mfma.hip still compiles a packed kernel of its own'


def test_packed_kernels_have_no_scratch():
    """The packed kernels owe their registers to the streaming kernels compiled beside them (csrc/attn_hd.hip says so at its top
    and above the packed kernels): compiled alone, or beside other neighbours, the backward kernels reach their register cap and
    spill.  No instantiation may have a private segment or a spilled register."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import check_isa
    _stubs()
    if not os.path.exists(check_isa.READELF):
        return
    packed = {k: v for k, v in check_isa.spill_counts(OBJ).items() if 'small_kernel' in k}
    assert len(packed) == 32
    assert not {k: v for k, v in packed.items() if any(v)}, 'spilled sgprs, spilled vgprs, private segment bytes per kernel'


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
    # head_dim 64 always, the other head dims under the attn_hd switch
    assert re.search(r'\(hd == 64 \|\| options\(\)\.attn_hd\) && attn_small_eligible\(dtype, mode, L, hd\)', route)
    assert route.index('options().attn_valu') < route.index('attn_small_eligible')             # attn_valu=1 still wins
    assert 'HDSMALL' not in route and 'hd_small' not in route
    kernels = read(PKG, 'csrc', 'attn_hd.hip')
    assert 'attn_fwd_small_launch' in kernels and 'attn_bwd_small_launch' in kernels and 'namespace hdsmall' not in kernels
    for gone in ('small_rows', 'SmallRows', 'attn_fwd_small_launch'):
        assert gone not in read(PKG, 'csrc', 'attn_mfma.hip'), f'csrc/attn_mfma.hip still has {gone}'
    hdr = read(ROOT, 'include', 'vtx.h')
    assert '"attn_hd" = mfma|valu' in hdr
    i = hdr.index('"attn_hd" = mfma|valu')
    assert 'up to 32 tokens' in hdr[i:i + 900], 'include/vtx.h: the attn_hd comment does not name the packed route'
    doc = read(ROOT, 'INTEGRATION.md')
    row = re.search(r'^\| `attn_hd` \| `VTX_ATTN_HD` \|.*$', doc, flags=re.M)
    assert row and 'up to 32 tokens' in row.group(0) and 'TIME_CLS' in row.group(0)
