"""Build libvtx.so, libvtx_aug.so, libvtx_randaug.so, libvtx_views.so, libvtx_mix.so, libvtx_stem.so, libvtx_ragged.so and libvtx_dropout.so (gfx950) with hipcc -- no torch headers, no cmake.

    python videotransformer-pytorch_amd/csrc/build.py [--force]

Each .hip file is compiled to an object (skipped when up to date) and linked into
videotransformer-pytorch_amd/libvtx.so; csrc/aug.hip (clip augmentation, include/vtx_aug.h) becomes
videotransformer-pytorch_amd/libvtx_aug.so and csrc/randaug.hip (RandAugment, include/vtx_randaug.h)
videotransformer-pytorch_amd/libvtx_randaug.so, csrc/views.hip (test-time views, include/vtx_views.h)
videotransformer-pytorch_amd/libvtx_views.so and csrc/mix.hip (Mixup / CutMix on uint8 clips, include/vtx_mix.h)
videotransformer-pytorch_amd/libvtx_mix.so, csrc/stem.hip (MaskFeat from uint8 clips: the Conv3d stem gather and the HOG of
selected frames, include/vtx_stem.h) videotransformer-pytorch_amd/libvtx_stem.so, csrc/ragged.hip (views of clips that differ in
source size, include/vtx_ragged.h) videotransformer-pytorch_amd/libvtx_ragged.so, csrc/dropout.hip (dropout without a stored
mask, include/vtx_dropout.h) videotransformer-pytorch_amd/libvtx_dropout.so.  hipcc cross-compiles without a GPU.
"""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.dirname(HERE)
OUT = os.path.join(PKG, 'libvtx.so')
AUG_OUT = os.path.join(PKG, 'libvtx_aug.so')
RANDAUG_OUT = os.path.join(PKG, 'libvtx_randaug.so')
VIEWS_OUT = os.path.join(PKG, 'libvtx_views.so')
MIX_OUT = os.path.join(PKG, 'libvtx_mix.so')
STEM_OUT = os.path.join(PKG, 'libvtx_stem.so')
RAGGED_OUT = os.path.join(PKG, 'libvtx_ragged.so')
DROPOUT_OUT = os.path.join(PKG, 'libvtx_dropout.so')
OBJ = os.path.join(HERE, '_obj')
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
SOURCES = ['api.hip', 'ln.hip', 'gemm_nt.hip', 'gemm_tn.hip', 'attn.hip', 'attn_mfma.hip', 'attn_long.hip', 'attn_f32.hip', 'elementwise.hip', 'hog.hip', 'optim.hip', 'head.hip', 'mvit.hip', 'wprod.hip', 'xattn_mfma.hip']
# (Round 6 tried -fno-slp-vectorize -- hipcc's SLP pass packs adjacent float32 multiplies / FMAs of the epilogues into v_pk_*
# instructions and pays for it with register shuffles; beside the partner wave's MFMAs a packed VALU instruction costs more than the
# two it replaces (MI355X_MICROARCH.md): step 128.24 -> 127.84 ms over three interleaved A/B rounds.  NOT adopted: without the packing
# the compiler fuses other multiply-add pairs, every bf16 result moves inside its rounding noise, and the noisiest statistic of the
# suite -- the 24-layer default-stream maximum -- landed on the wrong side of its bar.  `build.py --variant noslp -fno-slp-vectorize`.)
AUG_SOURCES = ['aug.hip']          # the second library: nothing of it is linked into libvtx.so
RANDAUG_SOURCES = ['randaug.hip']  # the third: libvtx_aug.so keeps its seven symbols
VIEWS_SOURCES = ['views.hip']      # the fourth: frame selection + resize + ThreeCrop in one launch
MIX_SOURCES = ['mix.hip']          # the fifth: CutMix on bytes, Mixup inside the patch gather
STEM_SOURCES = ['stem.hip']        # the sixth: the MViT stem gather from bytes, HOG of selected frames (hog_kernel.h, shared with hog.hip)
RAGGED_SOURCES = ['ragged.hip']    # the seventh: views.hip's kernel with per-clip base pointer and geometry
DROPOUT_SOURCES = ['dropout.hip']  # the eighth: mask, DropPath scale and residual in one launch, the mask regenerated in the backward
FLAGS = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-fno-gpu-rdc', '-Wno-unused-result', '-Wno-unused-value', '-Wno-inline-asm',
         '-Wno-cuda-compat']
EXTRA = {'hog.hip': ['-ffp-contract=off'],         # bit-exact HOG: no fma contraction
         'aug.hip': ['-ffp-contract=off'],         # torchvision's float32 blends and weighted sums, product by product
         'randaug.hip': ['-ffp-contract=off'],     # likewise: sharpness blend, autocontrast scale, warp coordinates
         'views.hip': ['-ffp-contract=off'],       # the weighted sums of aug.hip's resampler, byte for byte
         'mix.hip': ['-ffp-contract=off'],         # normalise then blend: five roundings per operand pair
         'stem.hip': ['-ffp-contract=off'],        # hog_kernel.h as hog.hip compiles it; normalise: three roundings per tap
         'ragged.hip': ['-ffp-contract=off'],      # views.hip's weighted sums, byte for byte
         'dropout.hip': ['-ffp-contract=off']}     # mask, scale, row scale, residual: four float32 operations, one rounding on the store


def _deps():
    hdrs = [os.path.join(HERE, f) for f in os.listdir(HERE) if f.endswith('.h')]
    hdrs.append(os.path.join(PKG, '..', 'include', 'vtx.h'))
    hdrs.append(os.path.join(PKG, '..', 'include', 'vtx_aug.h'))
    hdrs.append(os.path.join(PKG, '..', 'include', 'vtx_randaug.h'))
    hdrs.append(os.path.join(PKG, '..', 'include', 'vtx_views.h'))
    hdrs.append(os.path.join(PKG, '..', 'include', 'vtx_mix.h'))
    hdrs.append(os.path.join(PKG, '..', 'include', 'vtx_stem.h'))
    hdrs.append(os.path.join(PKG, '..', 'include', 'vtx_ragged.h'))
    hdrs.append(os.path.join(PKG, '..', 'include', 'vtx_dropout.h'))
    hdrs.append(os.path.abspath(__file__))                       # the flags live here
    return max(os.path.getmtime(h) for h in hdrs)


def _compile(src, force):
    obj = os.path.join(OBJ, src.replace('.hip', '.o'))
    spath = os.path.join(HERE, src)
    if (not force and os.path.exists(obj)
            and os.path.getmtime(obj) > max(os.path.getmtime(spath), _deps())):
        return obj, False
    cmd = [HIPCC] + FLAGS + EXTRA.get(src, []) + ['-c', spath, '-o', obj]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f'hipcc failed on {src}:\n{r.stdout}\n{r.stderr}')
    if r.stderr.strip():
        sys.stderr.write(r.stderr)
    return obj, True


def build_variant(name, defines):
    """An experimental build next to the product library: libvtx_<name>.so with -D<defines> (objects under _obj/<name>/);
    load it with VTX_LIB=<path> to A/B two builds on the same GPU box (tools/micro/*.sh).  Not part of build()."""
    obj_dir = os.path.join(OBJ, name)
    os.makedirs(obj_dir, exist_ok=True)
    out = os.path.join(PKG, f'libvtx_{name}.so')

    def one(src):
        obj = os.path.join(obj_dir, src.replace('.hip', '.o'))
        # (an entry that starts with '-' is passed to hipcc as it is: --variant noslp -fno-slp-vectorize)
        cmd = ([HIPCC] + FLAGS + EXTRA.get(src, []) + [d if d.startswith('-') else '-D' + d for d in defines] +
               ['-c', os.path.join(HERE, src), '-o', obj])
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f'hipcc failed on {src}:\n{r.stderr}')
        return obj
    with ThreadPoolExecutor(max_workers=min(8, len(SOURCES))) as ex:
        objs = list(ex.map(one, SOURCES))
    r = subprocess.run([HIPCC, '--offload-arch=gfx950', '-shared', '-fPIC', '-o', out] + objs, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f'link failed:\n{r.stderr}')
    return out


def build(force=False, verbose=True):
    """Compile what is stale and link.  Serialised across processes by a file lock: N ranks of a multi-GPU launch may all
    find the library stale at the same moment (a fresh copy of the tree) and must not write the same objects concurrently."""
    import fcntl
    os.makedirs(OBJ, exist_ok=True)
    with open(os.path.join(OBJ, '.lock'), 'w') as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        try:
            return _build_locked(force, verbose)
        finally:
            fcntl.flock(lock, fcntl.LOCK_UN)


def _link(out, res, extra, verbose):
    if any(c for _, c in res) or not os.path.exists(out):
        cmd = [HIPCC, '--offload-arch=gfx950', '-shared', '-fPIC'] + extra + ['-o', out] + [o for o, _ in res]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f'link failed:\n{r.stdout}\n{r.stderr}')
        if verbose:
            print(f'built {out}')
    elif verbose:
        print(f'{out} up to date')


def _build_locked(force, verbose):
    every = SOURCES + AUG_SOURCES + RANDAUG_SOURCES + VIEWS_SOURCES + MIX_SOURCES + STEM_SOURCES + RAGGED_SOURCES + DROPOUT_SOURCES
    with ThreadPoolExecutor(max_workers=min(8, len(every))) as ex:
        res = list(ex.map(lambda s: _compile(s, force), every))
    n, m = len(SOURCES), len(SOURCES) + len(AUG_SOURCES)
    k = m + len(RANDAUG_SOURCES)
    j = k + len(VIEWS_SOURCES)
    i = j + len(MIX_SOURCES)
    h = i + len(STEM_SOURCES)
    g = h + len(RAGGED_SOURCES)
    _link(OUT, res[:n], [], verbose)
    # -Bsymbolic: the library's own definitions of the helpers common.h declares, whatever else the process has loaded
    _link(AUG_OUT, res[n:m], ['-Wl,-Bsymbolic'], verbose)
    _link(RANDAUG_OUT, res[m:k], ['-Wl,-Bsymbolic'], verbose)
    _link(VIEWS_OUT, res[k:j], ['-Wl,-Bsymbolic'], verbose)
    _link(MIX_OUT, res[j:i], ['-Wl,-Bsymbolic'], verbose)
    _link(STEM_OUT, res[i:h], ['-Wl,-Bsymbolic'], verbose)
    _link(RAGGED_OUT, res[h:g], ['-Wl,-Bsymbolic'], verbose)
    _link(DROPOUT_OUT, res[g:], ['-Wl,-Bsymbolic'], verbose)
    return OUT


if __name__ == '__main__':
    if '--variant' in sys.argv:                         # python build.py --variant NAME DEFINE[=VALUE] ...
        i = sys.argv.index('--variant')
        print(build_variant(sys.argv[i + 1], sys.argv[i + 2:]))
    else:
        build(force='--force' in sys.argv)
