"""Host-side plumbing of the GEMM dispatch and the option table -- no GPU needed.

  1. vtx_gemm_tn_workspace(M, N1, N2) over a grid that crosses every threshold of the weight-gradient plan (the 256-row slab
     floor of tn_splits, the ring's 1024 rows, the ping-pong kernel's 4096 rows and 256-column multiples, the headline
     M = 150528) equals, number for number, what a library built from the parent commit returns (VTX_PARENT_LIB, the mechanism
     of tests/test_gpu_long_attention.py; skipped when it names no file).  Asked at tn_cus = 256 and 240: the slab count of the
     ping-pong partition, hence the workspace, depends on it.
  2. vtx_set_option: every option accepts its default; the edge values of every parse rule are accepted or rejected as the
     rule says (flags take any integer, attn_fused clamps, pp_epi takes any integer, pp_grid is a multiple of 8 in 8..4096,
     tn_cus 32..1024, enums take their names only) -- and, with VTX_PARENT_LIB, exactly as the parent build does.
  3. A process started with any VTX_* variable set to a value that does not parse still loads the library.

Every library is driven in a child process of its own through ctypes: two builds of libvtx.so export the same C++ symbols."""
import json
import os
import subprocess
import sys

import pytest

import conftest
from helpers import ROOT

LIB = os.path.join(ROOT, 'videotransformer-pytorch_amd', 'libvtx.so')
WS_M = (8, 255, 256, 1023, 1024, 4095, 4096, 4097, 150528)
WS_N = (8, 128, 136, 256, 768, 2304, 3072)
DEFAULTS = dict(conftest._OPTION_DEFAULTS, attn_long='1', attn_f32='mfma')
ENV = dict(gemm_nt='VTX_GEMM_NT', gemm_tn='VTX_GEMM_TN', gemm_nodma='VTX_GEMM_NODMA', tn_safe='VTX_TN_SAFE', tn_cus='VTX_TN_CUS',
           attn_valu='VTX_ATTN_VALU', attn_long='VTX_ATTN_LONG', attn_f32='VTX_ATTN_F32', attn_hw_fwd='VTX_ATTN_HW_FWD',
           attn_hw_bwd='VTX_ATTN_HW_BWD', attn_fused='VTX_ATTN_FUSED', attn_fwd_stream='VTX_ATTN_FWD_STREAM', attn_dkv='VTX_ATTN_DKV',
           pp_grid='VTX_GEMM_PP_GRID', pp_cg='VTX_GEMM_PP_CG', pp_epi='VTX_GEMM_PP_EPI', pp_cont='VTX_GEMM_PP_CONT', ln_rows='VTX_LN_ROWS')
# (option, value) -> accepted?  From the rules of vtx_set_option as they stand in include/vtx.h and csrc/common.h.
EDGES = [(n, v, True) for n in ('gemm_nodma', 'tn_safe', 'attn_valu', 'attn_long', 'attn_fwd_stream', 'pp_cont') for v in ('0', '1', '2', '-1', 'on', '')]
EDGES += [('attn_fused', v, True) for v in ('-5', '0', '2', '3', '99', 'x')]                       # clamps to 0..2
EDGES += [('pp_epi', v, True) for v in ('-1', '0', '1', '6', '1000000', 'x')]                      # any integer
EDGES += [('pp_grid', v, ok) for v, ok in (('8', True), ('4096', True), ('264', True), ('0', False), ('7', False), ('12', False), ('4104', False), ('x', False))]
EDGES += [('tn_cus', v, ok) for v, ok in (('32', True), ('240', True), ('1024', True), ('31', False), ('1025', False), ('-1', False), ('x', False))]
EDGES += [('attn_dkv', v, ok) for v, ok in (('0', True), ('4', True), ('-1', False), ('5', False))]
EDGES += [('ln_rows', v, ok) for v, ok in (('1', True), ('4', True), ('0', False), ('5', False), ('x', False))]
EDGES += [(n, v, ok) for n in ('attn_hw_fwd', 'attn_hw_bwd', 'pp_cg') for v, ok in (('0', True), ('1000', True), ('-1', False))]
EDGES += [('gemm_nt', v, ok) for v, ok in (('ring256x4k32', True), ('pp256', True), ('ring', False), ('0', False), ('', False), ('AUTO', False))]
EDGES += [('gemm_tn', v, ok) for v, ok in (('w4', True), ('ring', True), ('ring256x3', False), ('4', False), ('', False))]
EDGES += [('attn_f32', v, ok) for v, ok in (('valu', True), ('mfma', True), ('1', False), ('', False))]
EDGES += [('pp_trace', v, True) for v in ('0', '0x0', 'x')] + [('no_such_option', '1', False), ('pp_trac', '0', False)]

CHILD = r'''
import ctypes, json, sys
lib = ctypes.CDLL(sys.argv[1])
job = json.load(sys.stdin)
lib.vtx_gemm_tn_workspace.restype = ctypes.c_size_t
lib.vtx_gemm_tn_workspace.argtypes = [ctypes.c_int] * 3
lib.vtx_set_option.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
out = {'version': lib.vtx_version(), 'ws': {}, 'set': []}
for cus in job['tn_cus']:
    assert lib.vtx_set_option(b'tn_cus', cus.encode()) == 0
    out['ws'][cus] = [lib.vtx_gemm_tn_workspace(m, a, b) for m in job['M'] for a in job['N'] for b in job['N']]
for name, value in job['set']:
    out['set'].append(lib.vtx_set_option(name.encode(), value.encode()) == 0)
print(json.dumps(out))
'''


def drive(lib, job=None, env=None):
    job = dict(dict(tn_cus=[], M=[], N=[], set=[]), **(job or {}))
    r = subprocess.run([sys.executable, '-c', CHILD, lib], input=json.dumps(job), capture_output=True, text=True,
                       env=dict(os.environ, **(env or {})), timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.fixture(scope='module')
def built():
    import __graft_entry__ as ge
    ge.ensure_built()
    return LIB


def parent_lib():
    parent = os.environ.get('VTX_PARENT_LIB', '')
    return os.path.abspath(parent) if parent and os.path.isfile(parent) else None


def test_tn_workspace_equals_the_parent_builds(built):
    parent = parent_lib()
    if parent is None:
        pytest.skip('VTX_PARENT_LIB does not name a library built from the parent commit')
    job = dict(tn_cus=['256', '240'], M=WS_M, N=WS_N)
    new, old = drive(built, job), drive(parent, job)
    for cus in job['tn_cus']:
        shapes = [(m, a, b) for m in WS_M for a in WS_N for b in WS_N]
        diff = [(s, o, n) for s, o, n in zip(shapes, old['ws'][cus], new['ws'][cus]) if o != n]
        print(f'tn_cus={cus}: {len(shapes)} shapes, {len(diff)} differ')
        assert not diff, diff[:5]
        assert all(n > 0 for n in new['ws'][cus])


def test_every_option_accepts_its_default_and_the_edges_parse_as_documented(built):
    sets = [(n, v) for n, v in DEFAULTS.items()] + [(n, v) for n, v, _ in EDGES]
    got = drive(built, dict(set=sets))
    assert got['version'] == 230
    want = [True] * len(DEFAULTS) + [ok for _, _, ok in EDGES]
    assert [(s, g) for s, g, w in zip(sets, got['set'], want) if g != w] == []
    parent = parent_lib()
    if parent is not None:
        assert drive(parent, dict(set=sets))['set'] == got['set']
        print(f'{len(sets)} (option, value) pairs: the same outcome as the parent build')


def test_a_bad_environment_value_keeps_the_library_loading(built):
    assert sorted(ENV) == sorted(DEFAULTS)                # every option but pp_trace has a variable
    bad = {var: 'no-such-value' for var in ENV.values()}
    got = drive(built, dict(set=list(DEFAULTS.items())), env=bad)         # the first call reads the environment
    assert got['version'] == 230 and all(got['set'])
    for name, var in ENV.items():                         # ... and one at a time, with a value out of the option's range
        got = drive(built, dict(set=[(name, DEFAULTS[name])]), env={var: '-7'})
        assert got['set'] == [True], (name, var)
