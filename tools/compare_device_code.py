"""Is a change host-only?  Compare the gfx950 device code of two builds, object by object.

    python tools/compare_device_code.py OTHER_TREE [THIS_TREE]

For every csrc/_obj/<file>.o of both trees: extract the device code object (as tools/check_isa.py does), hash its .text section
and list its kernel symbols.  Prints one line per file (sha256 of .text, other / this) and exits 1 when a .text section or a
symbol list differs.  The whole code object is NOT compared: it carries the build directory, .text does not.  When the
sections differ but every kernel's own bytes agree (instantiations emitted in another order) the line says so; when the symbol
lists differ (a kernel was added or retired) it names, of the kernels both builds have, the ones whose bytes differ.
"""
import hashlib
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = os.environ.get('LLVM_BIN', '/opt/rocm/llvm/bin')
OBJ = os.path.join('videotransformer-pytorch_amd', 'csrc', '_obj')


def device_code(obj):
    """(.text bytes, {kernel symbol: its bytes}) of the device code object inside a host object."""
    tmp = tempfile.mkdtemp()
    try:
        local = os.path.join(tmp, 'k.o')
        shutil.copy(obj, local)
        subprocess.run([os.path.join(LLVM, 'llvm-objdump'), '--offloading', local], cwd=tmp, capture_output=True, check=False)
        dev = [f for f in os.listdir(tmp) if 'amdgcn' in f]
        if not dev:
            raise RuntimeError('no device code object found in ' + obj)
        co, text = os.path.join(tmp, dev[0]), os.path.join(tmp, 'text.bin')
        subprocess.run([os.path.join(LLVM, 'llvm-objcopy'), '-O', 'binary', '--only-section=.text', co, text], check=True)
        blob = open(text, 'rb').read()
        hdr = subprocess.run([os.path.join(LLVM, 'llvm-readelf'), '-S', '-W', co], capture_output=True, text=True, check=True).stdout
        base = next(int(l.split('.text')[1].split()[1], 16) for l in hdr.splitlines() if ' .text ' in l)
        syms = subprocess.run([os.path.join(LLVM, 'llvm-objdump'), '-t', co], capture_output=True, text=True, check=True).stdout
        kernels = {}
        for l in syms.splitlines():                       # address flags .text size [visibility] name
            f = l.split()
            if '.text' in f and 'F' in f[:f.index('.text')]:
                a, n = int(f[0], 16) - base, int(f[f.index('.text') + 1], 16)
                kernels[f[-1]] = blob[a:a + n]
        return blob, kernels
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    other = sys.argv[1]
    this = sys.argv[2] if len(sys.argv) > 2 else ROOT
    objs = [{f for f in os.listdir(os.path.join(t, OBJ)) if f.endswith('.o')} for t in (other, this)]
    bad = 0
    for n in sorted(objs[0] | objs[1]):
        if n not in objs[0] or n not in objs[1]:                # a source file was added or retired: its kernels have no partner here
            bad += 1
            print(f'{n:18s} ONLY IN {"THIS" if n in objs[1] else "THE OTHER"} TREE')
            continue
        ta, ka = device_code(os.path.join(other, OBJ, n))
        tb, kb = device_code(os.path.join(this, OBJ, n))
        ha, hb = hashlib.sha256(ta).hexdigest()[:16], hashlib.sha256(tb).hexdigest()[:16]
        if sorted(ka) != sorted(kb):
            common = sorted(set(ka) & set(kb))
            verdict = ('SYMBOLS DIFFER: ' + ' '.join(sorted(set(ka) ^ set(kb))) + f'; OF THE {len(common)} IN BOTH, DIFFERENT: ' +
                       (' '.join(k for k in common if ka[k] != kb[k]) or 'none'))
        elif ta == tb:
            verdict = 'identical'
        elif all(ka[k] == kb[k] for k in ka):
            verdict = 'identical per kernel symbol (emitted in another order)'
        else:
            verdict = 'DIFFERENT: ' + ' '.join(k for k in sorted(ka) if ka[k] != kb[k])
        bad += verdict.isupper() or verdict[:4].isupper()
        print(f'{n:18s} {len(ka):4d} symbols  .text {ha} / {hb}  {verdict}')
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
