"""The exact-fp32 MFMA attention kernels at head_dim 32, 96 and 128 (csrc/attn_hd_f32.hip) as compiled -- no GPU needed: the nine
instantiations are in the object, every matrix instruction in them is v_mfma_f32_32x32x2_f32, none has a private segment
(the file's header settles: no scratch anywhere); build.py names the source and the routing rows of the documents the route."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'videotransformer-pytorch_amd')
KERNELS = ['fwd_kernel', 'bwd_dq_kernel', 'bwd_dkv_kernel']
HDS = [32, 96, 128]
SCRATCH = {(k, hd): 0 for k in KERNELS for hd in HDS}                   # bytes of private segment per lane, as settled


def _symbol(kernel, hd):
    """the mangled name of vtx::hdf32::<kernel><hd> up to its template argument"""
    return f'_ZN3vtx5hdf32{len(kernel)}{kernel}ILi{hd}EEE'


@pytest.fixture(scope='module')
def isa():
    import __graft_entry__ as ge
    ge.ensure_built()
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import check_isa
    obj = os.path.join(PKG, 'csrc', '_obj', 'attn_hd_f32.o')
    assert os.path.exists(obj), 'csrc/attn_hd_f32.hip was not compiled'
    if not os.path.exists(check_isa.OBJDUMP):
        pytest.skip('needs llvm-objdump')
    bodies = dict(check_isa.kernels(check_isa.disassemble(obj)))
    notes = check_isa.spill_counts(obj) if os.path.exists(check_isa.READELF) else None
    return bodies, notes


@pytest.mark.parametrize('hd', HDS)
@pytest.mark.parametrize('kernel', KERNELS)
def test_instantiation_uses_the_fp32_mfma_only(kernel, hd, isa):
    bodies, _ = isa
    hit = [n for n in bodies if n.startswith(_symbol(kernel, hd))]
    assert len(hit) == 1, f'{kernel}<{hd}>: {len(hit)} kernels of that name in attn_hd_f32.o'
    mfma = re.findall(r'\bv_mfma_\w+', '\n'.join(bodies[hit[0]]))
    # one 32-row tile unrolled once: forward HD / 2 + HD / 2, dq 2 HD / 2 + HD / 2, dk / dv 2 HD / 2 + 2 HD / 2
    least = {'fwd_kernel': hd, 'bwd_dq_kernel': 3 * hd // 2, 'bwd_dkv_kernel': 2 * hd}[kernel]
    assert len(mfma) >= least, f'{kernel}<{hd}>: {len(mfma)} matrix instructions, a tile takes {least}'
    other = sorted(set(m for m in mfma if m != 'v_mfma_f32_32x32x2_f32'))
    assert not other, f'{kernel}<{hd}>: matrix instructions other than v_mfma_f32_32x32x2_f32: {other}'


@pytest.mark.parametrize('hd', HDS)
@pytest.mark.parametrize('kernel', KERNELS)
def test_private_segment_is_what_the_header_settles(kernel, hd, isa):
    _, notes = isa
    if notes is None:
        pytest.skip('needs llvm-readelf')
    hit = [v for n, v in notes.items() if n.startswith(_symbol(kernel, hd))]
    assert len(hit) == 1, f'{kernel}<{hd}>: {len(hit)} resource notes'
    sgpr_spills, vgpr_spills, scratch = hit[0]
    print(f'{kernel}<{hd}>: spilled sgpr {sgpr_spills}, vgpr {vgpr_spills}, private segment {scratch} B')
    assert scratch == SCRATCH[kernel, hd] and (scratch or vgpr_spills == 0)


def test_only_the_nine_kernels_are_in_the_object(isa):
    _, notes = isa
    if notes is None:
        pytest.skip('needs llvm-readelf')
    assert sorted(n.split('EEE')[0] + 'EEE' for n in notes) == sorted(_symbol(k, hd) for k in KERNELS for hd in HDS)


def test_build_and_documents_name_the_route():
    build = open(os.path.join(PKG, 'csrc', 'build.py')).read()
    sources = re.search(r'^SOURCES = \[(.*?)\]', build, flags=re.M | re.S).group(1)
    assert "'attn_hd_f32.hip'" in sources
    route = open(os.path.join(PKG, 'csrc', 'attn.hip')).read()
    assert 'attn_hd_f32_eligible' in route and 'attn_fwd_hd_f32_launch' in route and 'attn_bwd_hd_f32_launch' in route
    integ = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    row = re.search(r'^\| `attn_f32` \| `VTX_ATTN_F32` \|.*$', integ, flags=re.M).group(0)
    assert 'attn_hd_f32.hip' in row
    design = open(os.path.join(ROOT, 'DESIGN.md')).read()
    assert re.search(r'^\s*\|?\s*fp32\s*\|[^\n]*attn_hd_f32\.hip', design, flags=re.M), 'DESIGN.md 4.3: no routing row for attn_hd_f32.hip'
