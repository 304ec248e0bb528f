"""Tensor-level wrappers over the C ABI (one Python function per libvtx entry point).

PyTorch is used here only for device memory (``torch.empty``), the current HIP
stream and dtype bookkeeping; every FLOP on the path is issued by libvtx.so.
All tensors must be CUDA (HIP) tensors; CPU tensors raise -- there is no fallback.
"""
import ctypes as C

import torch

from . import _lib
from ._lib import RowMap, IDENT, GemmDesc, GemmTnDesc, AttnDesc, AttnBwdDesc, call  # noqa: F401

_DT = {torch.float32: _lib.VTX_F32, torch.bfloat16: _lib.VTX_BF16}


def dt(t):
    try:
        return _DT[t.dtype]
    except KeyError:
        raise TypeError(f'vtx: unsupported activation dtype {t.dtype} (float32 or bfloat16)')


def need_cuda(*ts):
    """Every operand must live on the CURRENT HIP device (kernels are launched on its current stream)."""
    cur = None
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError('vtx: the HIP path needs CUDA/HIP tensors (no CPU fallback); '
                               f'got a tensor on {t.device}')
        if cur is None:
            cur = torch.cuda.current_device()
        if t.device.index != cur:
            raise RuntimeError(f'vtx: tensor on {t.device} but the current device is cuda:{cur} '
                               '(wrap the call in torch.cuda.device(...))')


def ptr(t):
    return None if t is None else t.data_ptr()


def stream():
    return torch.cuda.current_stream().cuda_stream


def rowmap(grp=0, skip=0, base=0):
    return RowMap(int(grp), int(skip), int(base))


def tabmap(rows_per_group, table, max_step):
    """Table row map: logical row m -> m + table[m // rows_per_group] (``table``: int32 device tensor, one row offset per
    group plus a spare entry; ``max_step``: upper bound of the difference of two consecutive entries)."""
    need_cuda(table)
    if table.dtype != torch.int32:
        raise TypeError('tabmap: int32 table expected')
    return RowMap(int(rows_per_group), int(max_step), 0, table.data_ptr())


def upload_i32(values, device):
    """list / array of ints -> int32 device tensor, through the pinned-memory copy kernel of upload_f32 (bit copy)."""
    import numpy as np
    a = np.asarray(values, dtype=np.int32)
    return upload_f32(torch.from_numpy(a.view(np.float32)), device).view(torch.int32)


def tokmap(n_tokens):
    """logical token row (clip-major, no cls) -> physical row of a [B, 1+N, D] tensor."""
    return RowMap(int(n_tokens), 1, 1)


def clsmap(n_tokens):
    """logical row b -> physical row b*(1+N): the cls row of every clip."""
    return RowMap(1, int(n_tokens), 0)


# ---- optional per-launch timing (bench.py rooflines): HIP events on the launch stream ----
_prof = None


def profile_start(classes=('gemm_nt',)):
    """Time every launch of the named kernel classes with a pair of HIP events on the launch stream
    (torch.cuda.Event records on torch's current stream, which is the stream the kernels are launched on)."""
    global _prof
    _prof = {c: [] for c in classes}


def profile_stop():
    """-> {class: {shape_key: [launches, total_ms, flops, algorithmic_bytes]}}; call after torch.cuda.synchronize()."""
    global _prof
    out = {}
    for c, recs in (_prof or {}).items():
        per = out.setdefault(c, {})
        for e0, e1, key, fl, by in recs:
            r = per.setdefault(key, [0, 0.0, 0.0, 0.0])
            r[0] += 1
            r[1] += e0.elapsed_time(e1)
            r[2] += fl
            r[3] += by
    _prof = None
    return out


def profile_totals(per_class):
    """{class: {key: [n, ms, flops, bytes]}} -> {class: (n, ms, flops, bytes)}."""
    return {c: tuple(sum(v[i] for v in d.values()) for i in range(4)) for c, d in per_class.items()}


class _timed:
    def __init__(self, cls, flops=0.0, nbytes=0.0, key=''):
        self.on = _prof is not None and cls in _prof
        self.cls, self.rec = cls, (key, float(flops), float(nbytes))

    def __enter__(self):
        if self.on:
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e1 = torch.cuda.Event(enable_timing=True)
            self.e0.record()

    def __exit__(self, *a):
        if self.on:
            self.e1.record()
            _prof[self.cls].append((self.e0, self.e1) + self.rec)


def _f32(t):
    if t is not None and t.dtype != torch.float32:
        raise TypeError('vtx: parameter tensors must be float32')
    return t


# ------------------------------------------------------------------ LayerNorm
def layernorm_fwd(x, rows, D, ldx, xmap, gamma, beta, eps, y, ldy, ymap=IDENT, mean=None, rstd=None):
    need_cuda(x, y, gamma, beta)
    with _timed('ln_fwd', nbytes=rows * D * (x.element_size() + y.element_size()), key=f'{rows}x{D}'):
        call('vtx_layernorm_fwd', dt(x), rows, D, ptr(x), ldx, xmap, ptr(_f32(gamma)), ptr(_f32(beta)), float(eps),
             ptr(y), ldy, ymap, ptr(mean), ptr(rstd), stream())


def layernorm_acc_fwd(xs, d, rows, D, lds, smap, xo, ldo, omap, gamma=None, beta=None, eps=1e-5, y=None, ldy=0, ymap=IDENT,
                      mean=None, rstd=None):
    """The exact residual stream (vtx_layernorm_acc_fwd): xo = (xs or 0) + d in float32 on the mapped rows and, with ``y``, the
    LayerNorm of those rows (bf16).  xs: float32 stream or None; d: bf16 contribution in the stream layout."""
    need_cuda(d, xo, xs, y)
    if d.dtype != torch.bfloat16 or xo.dtype != torch.float32 or (xs is not None and xs.dtype != torch.float32):
        raise TypeError('layernorm_acc_fwd: d bfloat16, xs / xo float32')
    nb = rows * D * (2 + 4 + (4 if xs is not None else 0) + (2 if y is not None else 0))
    with _timed('ln_fwd', nbytes=nb, key=f'acc {rows}x{D}'):
        call('vtx_layernorm_acc_fwd', rows, D, ptr(xs), ptr(d), lds, smap, ptr(xo), ldo, omap, ptr(_f32(gamma)), ptr(_f32(beta)),
             float(eps), ptr(y), ldy, ymap, ptr(mean), ptr(rstd), stream())


def layernorm_bwd(dy, lddy, dymap, x, ldx, xmap, rows, D, mean, rstd, gamma, dres, dx, lddx, dgamma, dbeta, dres32=None, dx32=None):
    """dx = (dres or 0) + LN'(dy); with dres32 / dx32 (float32 gradient stream, bf16 kernels over the float32 stream x):
    dx32 = dres32 + LN'(dy) in float32, dx = bf16(dx32) (vtx_layernorm_bwd_g32; ``dres`` is not read)."""
    need_cuda(dy, x, dx)
    ws_bytes = _lib.load().vtx_layernorm_bwd_workspace(rows, D)
    ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device=x.device)
    if dres32 is not None:
        need_cuda(dres32, dx32)
        if dy.dtype != torch.bfloat16 or x.dtype != torch.float32 or dres32.dtype != torch.float32 or dx32.dtype != torch.float32:
            raise TypeError('layernorm_bwd: the float32 gradient stream takes bf16 dy / dx and float32 x / dres32 / dx32')
        with _timed('ln_bwd', nbytes=(2 + 4 + 4 + 4 + 2) * rows * D, key=f'g32 {rows}x{D}'):
            call('vtx_layernorm_bwd_g32', rows, D, ptr(dy), lddy, dymap, ptr(x), ldx, xmap, ptr(mean), ptr(rstd), ptr(gamma), ptr(dres32),
                 ptr(dx32), ptr(dx), lddx, ptr(dgamma), ptr(dbeta), ptr(ws), ws_bytes, stream())
        return
    # bf16 gradients with x stored as float32: the exact residual stream (vtx.set_stream('fp32'))
    mixed = dy.dtype == torch.bfloat16 and x.dtype == torch.float32
    with _timed('ln_bwd', nbytes=((3.0 if dres is not None else 2.0) * dy.element_size() + x.element_size()) * rows * D, key=f'{rows}x{D}'):
        call('vtx_layernorm_bwd', _lib.VTX_BF16_X32 if mixed else dt(dy), rows, D, ptr(dy), lddy, dymap, ptr(x), ldx, xmap, ptr(mean), ptr(rstd),
             ptr(gamma), ptr(dres), ptr(dx), lddx, ptr(dgamma), ptr(dbeta), ptr(ws), ws_bytes, stream())


# ----------------------------------------------------------------------- GEMM
_nt_ws = {}


def _gemm_nt_workspace(device):
    """Tile counters of the persistent GEMM: one zeroed buffer per (device, stream); the kernel leaves it
    zeroed, and launches on one stream are ordered, so it is never shared by two launches in flight."""
    key = (device.index, torch.cuda.current_stream(device).cuda_stream)
    ws = _nt_ws.get(key)
    if ws is None:
        ws = torch.zeros(_lib.load().vtx_gemm_nt_workspace() // 4, dtype=torch.int32, device=device)
        _nt_ws[key] = ws
    return ws


def gemm_nt(A, B, Cout, M, N, K, lda=None, ldb=None, ldc=None, amap=IDENT, cmap=IDENT, bias=None, act=0,
            C2=None, dgelu_in=None, dgelu_kind=0, row_scale=None, rs=(1, 0, 1, 0), R=None, ldr=None, rmap=IDENT,
            r_period=0, split_row=0, Csplit=None):
    """C = epilogue(A[M,K] @ B[N,K]^T); see vtx_gemm_nt in include/vtx.h."""
    need_cuda(A, B, Cout)
    if A.dtype != B.dtype or A.dtype != Cout.dtype:
        raise TypeError(f'gemm_nt: dtype mismatch {A.dtype} {B.dtype} {Cout.dtype}')
    d = GemmDesc()
    d.dtype = dt(A); d.M, d.N, d.K = int(M), int(N), int(K)
    d.A = ptr(A); d.lda = K if lda is None else lda; d.amap = amap
    d.B = ptr(B); d.ldb = K if ldb is None else ldb
    d.C = ptr(Cout); d.ldc = N if ldc is None else ldc; d.cmap = cmap
    d.bias = ptr(_f32(bias)); d.act = act
    d.C2 = ptr(C2); d.ldc2 = N
    d.dgelu_in = ptr(dgelu_in); d.ld_dgelu = N; d.dgelu_kind = int(dgelu_kind)
    d.row_scale = ptr(_f32(row_scale)); d.rs_d1, d.rs_m1, d.rs_d2, d.rs_m2 = [int(v) for v in rs]
    d.R = ptr(R); d.ldr = (N if ldr is None else ldr); d.rmap = rmap; d.r_period = int(r_period)
    d.split_row = int(split_row); d.Csplit = ptr(Csplit); d.ldsplit = N
    ws = _gemm_nt_workspace(A.device)
    d.workspace = ptr(ws); d.ws_bytes = ws.numel() * 4
    if _lib._TRACE:
        import sys
        sys.stderr.write(f'[vtx]   gemm_nt M={M} N={N} K={K} lda={d.lda} ldc={d.ldc} A={tuple(A.shape)} B={tuple(B.shape)} C={tuple(Cout.shape)} amap=({amap.grp},{amap.skip},{amap.base}) cmap=({cmap.grp},{cmap.skip},{cmap.base}) bias={bias is not None} rs={row_scale is not None} R={R is not None} split={split_row}\n')
    if _prof is not None and 'gemm_nt' in _prof:
        # algorithmic bytes: every operand the launch must touch once (A, weight, C, and what the epilogue
        # reads or writes besides: residual, GELU' input, pre-activation copy)
        es = A.element_size()
        nb = (M * K + N * K + M * N) * es
        tags = ''
        if C2 is not None:
            nb += M * N * es
            tags += '+preact' if act == 1 else "+gelu'out"
        if dgelu_in is not None:
            nb += M * N * es
            tags += "+gelu'" if dgelu_kind == 0 else '+mul'
        if R is not None:
            nb += (min(M, r_period) if r_period else M) * N * es
            tags += '+res'
        if row_scale is not None:
            tags += '+scale'
        with _timed('gemm_nt', 2.0 * M * N * K, nb, f'{M}x{N}x{K}{tags}'):
            call('vtx_gemm_nt', C.byref(d), stream())
    else:
        call('vtx_gemm_nt', C.byref(d), stream())


def gemm_tn(A, B, M, N1, N2, out=None, lda=None, ldb=None, amap=IDENT, bmap=IDENT, accumulate=False,
            want_colsum=False, colsum_out=None, colsum_accumulate=False):
    """out[N1,N2] (fp32) (+)= sum_m A[m,:N1]^T B[m,:N2]; with want_colsum (or a colsum_out buffer, optionally
    accumulated into) also returns sum_m A[m,:N1] (the bias gradient that always accompanies a weight gradient)."""
    need_cuda(A, B)
    if out is None:
        out = torch.empty(N1, N2, dtype=torch.float32, device=A.device)
    if colsum_out is not None:
        need_cuda(colsum_out)
        want_colsum = True
        cs = colsum_out
    else:
        cs = torch.empty(N1, dtype=torch.float32, device=A.device) if want_colsum else None
    ws_bytes = _lib.load().vtx_gemm_tn_workspace(M, N1, N2)
    ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device=A.device)
    d = GemmTnDesc()
    d.dtype = dt(A); d.M, d.N1, d.N2 = int(M), int(N1), int(N2)
    d.A = ptr(A); d.lda = N1 if lda is None else lda; d.amap = amap
    d.B = ptr(B); d.ldb = N2 if ldb is None else ldb; d.bmap = bmap
    d.C = ptr(out); d.ldc = N2; d.accumulate = int(bool(accumulate))
    d.workspace = ptr(ws); d.ws_bytes = ws_bytes
    d.colsum = ptr(cs); d.colsum_accumulate = int(bool(colsum_accumulate and colsum_out is not None))
    with _timed('gemm_tn', 2.0 * M * N1 * N2, M * (N1 + N2) * A.element_size() + N1 * N2 * 4, f'{M}x{N1}x{N2}'):
        call('vtx_gemm_tn', C.byref(d), stream())
    return (out, cs) if want_colsum else out


def wprod(A, B, ta=False, tb=False, out=None, alpha=1.0, accumulate=False, u=None, v=None, x=None, y=None, alpha_y=1.0,
          z=None, beta_z=0.0, y_accumulate=False):
    """out (+)= alpha * op(A) @ op(B) (+ u v^T) on contiguous fp32 matrices, op = transpose when ta / tb; with x also
    y (+)= alpha_y * op(A) @ x + beta_z * z (y is allocated when None).  Returns out, or (out, y).  See vtx_wprod."""
    need_cuda(A, B, out, u, v, x, y, z)
    for t in (A, B, out, u, v, x, y, z):
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous()):
            raise TypeError('wprod: contiguous float32 tensors expected')
    d = _lib.WprodDesc()
    ar, ac = A.shape
    br, bc = B.shape
    if ta:
        d.N1, K, d.a_rs, d.a_ks = ac, ar, 1, ac
    else:
        d.N1, K, d.a_rs, d.a_ks = ar, ac, ac, 1
    if tb:
        Kb, d.N2, d.b_ks, d.b_cs = bc, br, 1, bc
    else:
        Kb, d.N2, d.b_ks, d.b_cs = br, bc, bc, 1
    if K != Kb:
        raise ValueError(f'wprod: inner dimensions differ ({K} vs {Kb})')
    d.K = K
    if out is None:
        if accumulate:
            raise ValueError('wprod: accumulate needs an output tensor')
        out = torch.empty(d.N1, d.N2, dtype=torch.float32, device=A.device)
    if x is not None and y is None:
        if y_accumulate:
            raise ValueError('wprod: y_accumulate needs y')
        y = torch.empty(d.N1, dtype=torch.float32, device=A.device)
    d.A, d.B, d.C, d.ldc = ptr(A), ptr(B), ptr(out), d.N2
    d.alpha, d.accumulate = float(alpha), int(bool(accumulate))
    d.u, d.v, d.x, d.y, d.z = ptr(u), ptr(v), ptr(x), ptr(y), ptr(z)
    d.alpha_y, d.beta_z, d.y_accumulate = float(alpha_y), float(beta_z), int(bool(y_accumulate))
    with _timed('wprod', 2.0 * d.N1 * d.N2 * K, 4.0 * (d.N1 * K + K * d.N2 + d.N1 * d.N2), f'{d.N1}x{d.N2}x{K}'):
        call('vtx_wprod', C.byref(d), stream())
    return out if x is None else (out, y)


def colsum(A, M, N, lda=None, amap=IDENT, out=None, accumulate=False):
    need_cuda(A)
    if out is None:
        out = torch.empty(N, dtype=torch.float32, device=A.device)
    ws_bytes = _lib.load().vtx_colsum_workspace(M, N)
    ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device=A.device)
    with _timed('colsum', nbytes=1.0 * M * N * A.element_size(), key=f'{M}x{N}'):
        call('vtx_colsum', dt(A), M, N, ptr(A), N if lda is None else lda, amap, ptr(out), int(bool(accumulate)),
             ptr(ws), ws_bytes, stream())
    return out


# ------------------------------------------------------------------ attention
def _attn_desc(qkv, out, lse, mode, S, L, H, hd, scale, B=0, T=0, P=0, probs=None):
    d = AttnDesc()
    d.dtype = dt(qkv); d.mode = mode
    d.S, d.L, d.H, d.hd = int(S), int(L), int(H), int(hd)
    d.B, d.T, d.P = int(B), int(T), int(P)
    d.qkv = ptr(qkv); d.ld_qkv = 3 * H * hd
    d.out = ptr(out); d.ld_out = H * hd
    d.lse = ptr(lse); d.probs = ptr(probs); d.scale = float(scale)
    return d


def _attn_kind(mode, L):
    """Timing class of a launch: the two spatial layouts, else by length."""
    if mode in (_lib.ATTN_SPACE, _lib.ATTN_SPACE_NOCLS):
        return 'space'
    return 'time' if L <= 32 else 'seq' if L <= 256 else 'long'


def attn_fwd(qkv, out, lse, mode, S, L, H, hd, scale, B=0, T=0, P=0, probs=None):
    need_cuda(qkv, out, lse)
    d = _attn_desc(qkv, out, lse, mode, S, L, H, hd, scale, B, T, P, probs)
    kind = _attn_kind(mode, L)
    rows = S * L                       # algorithmic bytes: read q,k,v, write o (+ fp32 log-sum-exp)
    with _timed(f'attn_fwd_{kind}', 4.0 * S * H * L * L * hd, rows * H * hd * 4 * qkv.element_size() + rows * H * 4,
                f'{S}x{L}x{H}'):
        call('vtx_attn_fwd', C.byref(d), stream())


def attn_bwd(qkv, out, lse, dout, dqkv, mode, S, L, H, hd, scale, B=0, T=0, P=0, dqkv_cls=None):
    need_cuda(qkv, out, dout, dqkv)
    b = AttnBwdDesc()
    b.f = _attn_desc(qkv, out, lse, mode, S, L, H, hd, scale, B, T, P)
    b.dout = ptr(dout); b.ld_dout = H * hd
    b.dqkv = ptr(dqkv); b.ld_dqkv = 3 * H * hd
    b.dqkv_cls = ptr(dqkv_cls)
    delta = torch.empty(S * H * L, dtype=torch.float32, device=qkv.device)
    b.delta = ptr(delta)
    kind = _attn_kind(mode, L)
    rows = S * L                       # read q,k,v,o,do, write dq,dk,dv
    with _timed(f'attn_bwd_{kind}', 10.0 * S * H * L * L * hd, rows * H * hd * 8 * qkv.element_size() + rows * H * 4,
                f'{S}x{L}x{H}'):
        call('vtx_attn_bwd', C.byref(b), stream())


# ------------------------------------------------------------------- glue ops
def fact_glue_fwd(x, time_embed, B, T, P, D):
    """ViViT fact_encoder glue: x [(B T), 1 + P, D] -> h [B, 1 + T, D] (vtx_fact_glue_fwd)."""
    need_cuda(x, time_embed)
    h = torch.empty(B, 1 + T, D, dtype=x.dtype, device=x.device)
    call('vtx_fact_glue_fwd', dt(x), B, T, P, D, ptr(x), ptr(_f32(time_embed)), ptr(h), stream())
    return h


def fact_glue_bwd(dh, B, T, P, D, d_time_embed=None, accumulate=False):
    need_cuda(dh)
    dx = torch.empty(B * T, 1 + P, D, dtype=dh.dtype, device=dh.device)
    call('vtx_fact_glue_bwd', dt(dh), B, T, P, D, ptr(dh), ptr(dx), ptr(d_time_embed), int(bool(accumulate)), stream())
    return dx


def cls_mean_fwd(a_cls, x, out, B, T, D, rows_per_clip):
    call('vtx_cls_mean_fwd', dt(out), B, T, D, ptr(a_cls), D, ptr(x), ptr(out), D, rows_per_clip, stream())     # x None: the mean alone


def space_grad_prep(dout, s, da, B, T, P, D):
    call('vtx_space_grad_prep', dt(dout), B, T, P, D, ptr(dout), D, ptr(s), ptr(da), D, stream())


def time_cls_grad_prep(dout, s, da, B, T, P, D):
    """Backward prep of temporal attention over the cls token: da[0:B*N] = dout[b, 1+n] * s[b*P + n/T], da[B*N + b*P + p] =
    dout[b, 0] * s[b*P + p] / P (s may be None).  vtx_space_grad_prep in its sequence-major form: P sequences per clip in the
    entry point's T slot, minus the T consecutive tokens of a sequence in its P slot (include/vtx.h)."""
    call('vtx_space_grad_prep', dt(dout), B, P, -T, D, ptr(dout), D, ptr(s), ptr(da), D, stream())


def cls_qkv_reduce(dqkv_cls, dqkv, B, T, W, rows_per_clip):
    call('vtx_cls_qkv_reduce', dt(dqkv), B, T, W, ptr(dqkv_cls), W, ptr(dqkv), W, rows_per_clip, stream())


def row_scale_copy(src, dst, rows, D, lds=None, smap=IDENT, ldd=None, dmap=IDENT, s=None, rs=(1, 0, 1, 0)):
    need_cuda(src, dst)
    call('vtx_row_scale_copy', dt(src), rows, D, ptr(src), D if lds is None else lds, smap, ptr(dst),
         D if ldd is None else ldd, dmap, ptr(s), int(rs[0]), int(rs[1]), int(rs[2]), int(rs[3]), stream())


# ---- dropout without a stored mask (libvtx_dropout.so: include/vtx_dropout.h, vtx_dropout_rows) ----
# csrc/dropout.hip caps its grid at DROPOUT_GRID_CAP workgroups of DROPOUT_BLOCK threads, 8 elements each: a launch of more
# than DROPOUT_TRIP elements strides (the tests cross the cap by these numbers).
DROPOUT_GRID_CAP, DROPOUT_BLOCK = 4096, 256
DROPOUT_TRIP = DROPOUT_GRID_CAP * DROPOUT_BLOCK * 8


def dropout_params(p):
    """(thr, scale) of a dropout probability: an element is dropped iff its 32-bit Philox word < thr = floor(p * 2^32) (Python
    integers), a kept one is multiplied by scale = float32(1) / float32(1 - p) -- transformer._keep_scale's arithmetic; 0 for p == 1."""
    import fractions
    import numpy as np
    p = float(p)
    if not 0.0 <= p <= 1.0:
        raise ValueError(f'dropout probability has to be between 0 and 1, but got {p}')
    thr = int(fractions.Fraction(p) * (1 << 32))          # floor of the exact product: p is a binary fraction
    scale = 0.0 if p == 1.0 else float(np.float32(1.0) / np.float32(1 - p))
    return thr, scale


def dropout_rows(x, y, rows, D, p, seed, site, e0=0, ldx=None, xmap=IDENT, ldy=None, ymap=IDENT, post=None, ldp=None, pmap=IDENT,
                 pre=None, pre_period=0, s=None, rs=(1, 0, 1, 0)):
    """y[ymap(m)] = post[pmap(m)] + s(m) * dropout(x[xmap(m)] + pre[m % pre_period]); the mask of element (m, c) is a function
    of (seed, site, e0 + m * D + c, p) alone.  y may be x (same maps)."""
    need_cuda(x, y, post, pre, s)
    thr, scale = dropout_params(p)
    if post is not None and post.dtype != x.dtype:
        raise TypeError('dropout_rows: the residual must have the dtype of x')
    _lib.dropout_call('vtx_dropout_rows', dt(x), int(rows), int(D), ptr(x), D if ldx is None else ldx, xmap, ptr(y), D if ldy is None else ldy,
         ymap, ptr(post), D if ldp is None else ldp, pmap, ptr(_f32(pre)), int(pre_period), ptr(_f32(s)), int(rs[0]), int(rs[1]),
         int(rs[2]), int(rs[3]), thr, scale, int(seed), int(site), int(e0), stream())


def dropped_rows_fix(s, M, D, group_rows, x=None, xmap=IDENT, bias=None, out=None, omap=IDENT, zero=None, ldx=None, ldo=None):
    """Rows of the groups with s == 0: out[omap(m)] = x[xmap(m)] + bias; zero[m] = 0 (either part optional)."""
    ref = out if out is not None else zero
    need_cuda(ref, s)
    call('vtx_dropped_rows_fix', dt(ref), M, D, group_rows, ptr(s), ptr(x), D if ldx is None else ldx, xmap, ptr(bias),
         ptr(out), D if ldo is None else ldo, omap, ptr(zero), D, stream())


def dropped_rows_colsum(src, s, M, D, group_rows, smap=IDENT, lds=None, nparts=96):
    """[nparts, D] fp32 partial column sums of src over the rows of the groups with s == 0."""
    need_cuda(src, s)
    part = torch.empty((nparts, D), dtype=torch.float32, device=src.device)
    call('vtx_dropped_rows_colsum', dt(src), M, D, group_rows, ptr(s), ptr(src), D if lds is None else lds, smap, ptr(part),
         nparts, stream())
    return part


def reduce_rows(inp, nj, ni, D, ld, base, si, sj, out=None, scale=1.0, accumulate=False):
    need_cuda(inp)
    if out is None:
        out = torch.empty(nj, D, dtype=torch.float32, device=inp.device)
    call('vtx_reduce_rows', dt(inp), nj, ni, D, ptr(inp), ld, base, si, sj, ptr(out), D, float(scale),
         int(bool(accumulate)), stream())
    return out


def cast_transpose(W, dtype, want_c=True, want_t=True):
    """fp32 [R,C] parameter -> (Wc [R,C], WcT [C,R]) in `dtype` (fp32: Wc is W itself)."""
    need_cuda(W)
    if W.dtype != torch.float32:
        raise TypeError(f'vtx: cast_transpose stages fp32 weights, got {W.dtype}')
    R, Cc = W.shape
    W = W.contiguous()
    code = _DT[dtype]
    Wc = None
    if want_c:
        Wc = W if dtype == torch.float32 else torch.empty(R, Cc, dtype=dtype, device=W.device)
    WcT = torch.empty(Cc, R, dtype=dtype, device=W.device) if want_t else None
    wc_arg = None if (Wc is None or Wc is W) else Wc
    if wc_arg is not None or WcT is not None:
        call('vtx_cast_transpose', code, R, Cc, ptr(W), ptr(wc_arg), ptr(WcT), stream())
    return Wc, WcT


def ct_table(entries, device):
    """Device table for mt_cast_transpose: entries = [(W fp32 [R,C] contiguous, Wc or None, WcT or None), ...].
    Returns (table tensor, tile prefix sums tensor, total tiles)."""
    tab = (_lib.CtTensor * len(entries))()
    starts = [0]
    for i, (W, wc, wt) in enumerate(entries):
        need_cuda(W)
        if not W.is_contiguous() or W.dtype != torch.float32:
            raise ValueError('ct_table: contiguous float32 matrices expected')
        R, Cc = W.shape
        tab[i].src, tab[i].dst_c, tab[i].dst_t = W.data_ptr(), ptr(wc), ptr(wt)
        tab[i].rows, tab[i].cols = R, Cc
        starts.append(starts[-1] + ((R + 63) // 64) * ((Cc + 63) // 64))
    tab_dev = torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8).to(device)
    starts_dev = torch.tensor(starts, dtype=torch.int32).to(device)
    return tab_dev, starts_dev, starts[-1]


def mt_cast_transpose(dtype, tab_dev, starts_dev, n_tensors, n_tiles):
    call('vtx_mt_cast_transpose', _DT[dtype], ptr(tab_dev), ptr(starts_dev), int(n_tensors), int(n_tiles), stream())


def cast_from_f32(src, dtype):
    need_cuda(src)
    if dtype == torch.float32:
        return src
    dst = torch.empty(src.shape, dtype=dtype, device=src.device)
    call('vtx_cast_from_f32', _DT[dtype], src.numel(), ptr(src.contiguous()), ptr(dst), stream())
    return dst


def cast_to_f32(src):
    need_cuda(src)
    if src.dtype == torch.float32:
        return src
    dst = torch.empty(src.shape, dtype=torch.float32, device=src.device)
    call('vtx_cast_to_f32', dt(src), src.numel(), ptr(src.contiguous()), ptr(dst), stream())
    return dst


# ---- small host -> device uploads without the copy engine --------------------------------------
# hipMemcpyAsync of tiny buffers interleaved with kernels stalls this stack badly (measured: 33
# DropPath mask uploads per step turned a 43 ms step into ~100 ms with 90 ms host stalls).  Instead
# the values are written into pinned host memory and a copy KERNEL on the compute stream reads them
# over the fabric.  Pinned slots are recycled only after the event recorded behind their kernel.
_pinned_slots = []          # [pinned tensor, event or None]


def upload_f32(values_cpu, device):
    """float32 CPU tensor (any shape) -> 1-D device tensor, stream-ordered, no memcpy call."""
    n = values_cpu.numel()
    slot = None
    for sl in _pinned_slots:
        if sl[0].numel() >= n and (sl[1] is None or sl[1].query()):
            slot = sl
            break
    if slot is None:
        cap = max(1024, 1 << (n - 1).bit_length())
        slot = [torch.empty(cap, dtype=torch.float32, pin_memory=True), None]
        _pinned_slots.append(slot)
    slot[0].numpy()[:n] = values_cpu.reshape(-1).numpy()        # NumPy copy: keep ATen's CPU thread pool out of the step
    out = torch.empty(n, dtype=torch.float32, device=device)
    call('vtx_cast_from_f32', _lib.VTX_F32, n, slot[0].data_ptr(), out.data_ptr(), stream())
    ev = torch.cuda.Event()
    ev.record()
    slot[1] = ev
    return out


_input_norm = None          # (mean[3], std[3]) applied to uint8 clips (set_input_normalization)


def set_input_normalization(mean, std):
    """Mean / std of the reference's transforms.Normalize for uint8 [B,T,H,W,3] clips (the values the
    reference is configured with, e.g. model_pretrain.py's --mean/--std); None disables uint8 input."""
    global _input_norm
    if mean is None:
        _input_norm = None
        return
    mean, std = [float(v) for v in mean], [float(v) for v in std]
    if len(mean) != 3 or len(std) != 3 or any(v == 0.0 for v in std):
        raise ValueError('set_input_normalization: need 3 means and 3 non-zero stds')
    _input_norm = (mean, std)


class MixedClip:
    """The Mixup of a decoded uint8 batch, not yet computed: stands for the float batch
    ``n(clip) * lam + n(clip.flip(0)) * (1 - lam)`` the reference's Mixup would have produced from the normalised clips
    (mixup.py:111-113; n = ToTensor + Normalize, set_input_normalization).  A mixed clip has no uint8 form and is never
    stored: the patch gather reads both partners and writes the mixed rows (patch_rows -> vtx_patch_rows_mix_u8).
    A plain carrier, not a tensor: ``clip`` (contiguous uint8 CUDA [B,T,H,W,3], B even -- not copied, not modified) and
    ``lam`` (float64).  TimeSformer and ViViT take it wherever they take a uint8 clip."""
    __slots__ = ('clip', 'lam')

    def __init__(self, clip, lam):
        if not isinstance(clip, torch.Tensor) or clip.dtype != torch.uint8:
            raise TypeError(f'MixedClip: a uint8 tensor is required, got {getattr(clip, "dtype", type(clip).__name__)}')
        if clip.ndim != 5 or clip.shape[-1] != 3:
            raise ValueError(f'MixedClip: the clip must be [B,T,H,W,3], got {tuple(clip.shape)}')
        if clip.shape[0] % 2:
            raise ValueError(f'MixedClip: clip b is mixed with clip B-1-b, the batch size must be even, got {clip.shape[0]}')
        if not clip.is_contiguous():
            raise ValueError('MixedClip: the clip must be contiguous')
        need_cuda(clip)
        self.clip, self.lam = clip, float(lam)

    shape = property(lambda self: self.clip.shape)
    device = property(lambda self: self.clip.device)
    dtype = property(lambda self: self.clip.dtype)
    is_cuda = property(lambda self: self.clip.is_cuda)

    def __len__(self):
        return len(self.clip)

    def __repr__(self):
        return f'MixedClip(uint8 {tuple(self.clip.shape)} on {self.clip.device}, lam={self.lam!r})'


#: (matrix, full_range) -> (y_off, c_y, c_rv, c_gu, c_gv, c_bu) of include/vtx_yuv.h: each within one step of its float64 matrix
#: rounded once, over all 2^24 triples (tests/test_yuv_host.py)
YUV_MATRICES = {('bt601', False): (16, 298, 409, 100, 208, 516), ('bt709', False): (16, 298, 459, 55, 136, 541),
                ('bt601', True): (0, 256, 359, 88, 183, 454), ('bt709', True): (0, 256, 403, 48, 120, 475)}


def _plane_stride(t, dim, default):
    """Stride of ``dim`` in elements; an axis of one element has no stride worth reading."""
    return int(t.stride(dim)) if t.shape[dim] > 1 else int(default)


#: the same table for 10-bit samples (include/vtx_yuv10.h): 12 fractional bits, ``yuv10_matrix`` of the two standards; each within
#: one step of its float64 matrix rounded once (tests/test_yuv10_host.py)
YUV10_MATRICES = {('bt601', False): (64, 1192, 1634, 401, 832, 2066), ('bt709', False): (64, 1192, 1836, 218, 546, 2163),
                  ('bt601', True): (0, 1021, 1431, 351, 729, 1809), ('bt709', True): (0, 1021, 1608, 191, 478, 1895)}
#: depth -> (largest y_off, largest |c|) of its conversion contract
_YUV_BOUNDS = {8: (255, 4096), 10: (1023, 16384)}


def yuv10_matrix(kr, kb, full_range=False):
    """Luma weights (Kr, Kb) of a standard -> the six integers (y_off, c_y, c_rv, c_gu, c_gv, c_bu) of the 10-bit contract
    (include/vtx_yuv10.h): floor(4096 * k + 0.5) of the float64 matrix -- limited range: luma 64 .. 940 scaled by 255 / 876, chroma
    by 255 / 896; full range: 255 / 1023 for both.  (0.299, 0.114) and (0.2126, 0.0722) give ``YUV10_MATRICES``; BT.2020 is
    (0.2627, 0.0593)."""
    import math
    kr, kb = float(kr), float(kb)
    kg = 1.0 - kr - kb
    if not (0.0 < kr < 1.0 and 0.0 < kb < 1.0 and kg > 0.0):
        raise ValueError(f'yuv10_matrix: luma weights kr={kr}, kb={kb} must be positive and sum to less than 1')
    sy, sc = (255.0 / 1023.0, 255.0 / 1023.0) if full_range else (255.0 / 876.0, 255.0 / 896.0)
    ks = (sy, 2.0 * (1.0 - kr) * sc, 2.0 * kb * (1.0 - kb) / kg * sc, 2.0 * kr * (1.0 - kr) / kg * sc, 2.0 * (1.0 - kb) * sc)
    return (0 if full_range else 64,) + tuple(int(math.floor(4096.0 * k + 0.5)) for k in ks)


class YUVClip:
    """A decoded 4:2:0 clip as the decoder left it, for the resampler to convert tap by tap (include/vtx_yuv.h has the
    contract): ``y`` uint8 [Ts,Hs,Ws]; I420: ``u`` and ``v`` uint8 [Ts,Hc,Wc]; NV12 (``v=None``): ``u`` the interleaved uint8
    [Ts,Hc,Wc,2] plane; Hc = (Hs + 1) // 2, Wc = (Ws + 1) // 2, odd sizes allowed.  Device tensors on the current device, read
    in place: row pitches and frame strides are the tensors' strides (a decoder's padded line size is a slice of the wider
    buffer), only the innermost stride is fixed: 1, and 2 for NV12's chroma columns.  ``matrix``: 'bt601' (the default: what
    swscale assumes for an untagged stream) or 'bt709', limited range unless ``full_range``; or six integers (y_off, c_y, c_rv,
    c_gu, c_gv, c_bu), 0 <= y_off <= 255 and |c| <= 4096.  Byte parity with a particular decoder's own RGB output is not
    claimed (chroma upsampling, rounding and dither differ among them).

    ``depth=10`` (include/vtx_yuv10.h): the same shapes of int16 or uint16 planes (the bits are read as unsigned), one 16-bit
    word per sample; ``v=None`` is then P010's interleaved plane, three planes are yuv420p10le.  ``msb_aligned``: the sample
    sits in the upper 10 bits of its word (True, what P010 says) or the lower 10 (False, yuv420p10le); None takes what the
    layout says.  The other bits of a word are ignored.  The presets are then the 10-bit ones (``YUV10_MATRICES``), six
    integers obey 0 <= y_off <= 1023 and |c| <= 16384 (``yuv10_matrix`` makes them from a standard's luma weights).

    A plain carrier like MixedClip, not a tensor: ``vtx.aug.ClipAugment`` / ``ClipEval`` / ``ClipTest`` take a list of them
    -- 8-bit and 10-bit clips in one list -- wherever they take a list of uint8 clips; ``ops.yuv420_to_rgb_u8`` gives the RGB
    frames.  The models, Mixup and hog_targets take the resampler's RGB output, not this."""
    __slots__ = ('y', 'u', 'v', 'matrix', 'depth', 'shift')

    def __init__(self, y, u, v=None, matrix='bt601', full_range=False, depth=8, msb_aligned=None):
        if isinstance(depth, bool) or depth not in (8, 10):
            raise ValueError(f'YUVClip: depth must be 8 or 10, got {depth!r} (12-bit and deeper content is not supported)')
        if msb_aligned is not None and not isinstance(msb_aligned, bool):
            raise ValueError(f'YUVClip: msb_aligned must be True, False or None, got {msb_aligned!r}')
        if depth == 8 and msb_aligned:
            raise ValueError('YUVClip: msb_aligned goes with depth=10: an 8-bit sample fills its byte')
        dtypes, named = ((torch.uint8,), 'a uint8 tensor') if depth == 8 else ((torch.int16, torch.uint16), 'an int16 or uint16 tensor at depth=10')
        size = 1 if depth == 8 else 2                            # bytes of a sample
        planes = [('y', y), ('u', u)] + ([] if v is None else [('v', v)])
        for n, p in planes:
            if not isinstance(p, torch.Tensor) or p.dtype not in dtypes:
                raise TypeError(f'YUVClip: {n} must be {named}, got {getattr(p, "dtype", type(p).__name__)}')
        if y.ndim != 3 or y.numel() == 0:
            raise ValueError(f'YUVClip: y must be a non-empty [Ts,Hs,Ws], got {tuple(y.shape)}')
        Ts, Hs, Ws = y.shape
        Hc, Wc = (Hs + 1) // 2, (Ws + 1) // 2
        want = (Ts, Hc, Wc, 2) if v is None else (Ts, Hc, Wc)
        for n, p in planes[1:]:
            if tuple(p.shape) != want:
                raise ValueError(f'YUVClip: {n} must be {want} for a luma of {(Ts, Hs, Ws)}' + (' (NV12: v=None)' if v is None else '') +
                                 f', got {tuple(p.shape)}')
        if v is None:
            inner = (_plane_stride(u, 3, 1), _plane_stride(u, 2, 2))
            if inner != (1, 2):
                raise ValueError(f'YUVClip: the {"NV12" if size == 1 else "P010"} plane must have U and V adjacent and chroma columns 2 '
                                 f'{"bytes" if size == 1 else "samples"} apart, got strides {u.stride()}')
        for n, p in planes if v is not None else planes[:1]:
            if _plane_stride(p, 2, 1) != 1:
                raise ValueError(f'YUVClip: the innermost stride of {n} must be 1, got strides {p.stride()}')
        if v is not None and [_plane_stride(u, d, 0) for d in (0, 1)] != [_plane_stride(v, d, 0) for d in (0, 1)]:
            raise ValueError(f'YUVClip: u and v must share their row pitch and frame stride, got strides {u.stride()} and {v.stride()}')
        for n, p, row in [('y', y, Ws), ('u', u, Wc * (2 if v is None else 1))]:
            pitch, frame = _plane_stride(p, 1, row) * size, _plane_stride(p, 0, 0) * size
            if pitch < row * size or not 0 <= frame < 2 ** 31 or pitch >= 2 ** 31:
                raise ValueError(f'YUVClip: {n}: a row pitch of {pitch} (rows of {row * size} bytes) and a frame stride of {frame} are not supported: '
                                 f'pitch >= row, 0 <= frame stride < 2^31')
        presets = YUV_MATRICES if depth == 8 else YUV10_MATRICES
        if isinstance(matrix, str):
            if (matrix, bool(full_range)) not in presets:
                raise ValueError(f"YUVClip: matrix {matrix!r}: 'bt601', 'bt709' or six integers")
            m = presets[(matrix, bool(full_range))]
        else:
            try:
                m = tuple(matrix)
            except TypeError:
                raise TypeError(f"YUVClip: matrix must be 'bt601', 'bt709' or six integers, got {type(matrix).__name__}") from None
            if len(m) != 6 or any(isinstance(c, bool) or not isinstance(c, int) for c in m):
                raise TypeError(f'YUVClip: matrix must be six integers (y_off, c_y, c_rv, c_gu, c_gv, c_bu), got {m!r}')
            y_max, c_max = _YUV_BOUNDS[depth]
            if not 0 <= m[0] <= y_max or any(abs(c) > c_max for c in m[1:]):
                raise ValueError(f'YUVClip: matrix {m}: 0 <= y_off <= {y_max} and |c| <= {c_max} keep the int32 sums in range')
        need_cuda(y, u, v)
        self.y, self.u, self.v, self.matrix, self.depth = y, u, v, m, depth
        self.shift = 6 if depth == 10 and (v is None if msb_aligned is None else msb_aligned) else 0

    nv12 = property(lambda self: self.v is None)                 # the interleaved layout: NV12, or P010 at depth 10
    planes = property(lambda self: (self.y, self.u) if self.v is None else (self.y, self.u, self.v))
    shape = property(lambda self: tuple(self.y.shape))
    device = property(lambda self: self.y.device)

    def __len__(self):
        return self.y.shape[0]

    @property
    def source_bytes(self):
        """Bytes of the samples of one frame: the luma and two quarter-size chroma planes, 1 or 2 bytes each."""
        _, Hs, Ws = self.shape
        return (Hs * Ws + 2 * ((Hs + 1) // 2) * ((Ws + 1) // 2)) * (2 if self.depth == 10 else 1)

    def record(self, Wr=0):
        """The clip's vtx_yuv420_clip record (include/vtx_yuv.h) as int32 [22]; ``Wr``: the columns of its resized row.  Of an
        8-bit clip (``record10`` serves both depths)."""
        import numpy as np
        Ts, Hs, Ws = self.shape
        step = 2 if self.nv12 else 1
        ptrs = np.array([self.y.data_ptr(), self.u.data_ptr(), self.u.data_ptr() + 1 if self.nv12 else self.v.data_ptr()], dtype=np.uint64)
        nums = [Ts, Hs, Ws, int(Wr), _plane_stride(self.y, 1, Ws), _plane_stride(self.y, 0, 0),
                _plane_stride(self.u, 1, (Ws + 1) // 2 * step), _plane_stride(self.u, 0, 0), step] + list(self.matrix) + [0]
        return np.concatenate([ptrs.view(np.int32), np.array(nums, dtype=np.int32)])

    def record10(self, Wr=0):
        """The clip's vtx_yuv10_clip record (include/vtx_yuv10.h) as int32 [24], of a clip of either depth: pitches and frame
        strides in bytes, the chroma step in samples, depth, shift."""
        import numpy as np
        Ts, Hs, Ws = self.shape
        step, size = 2 if self.nv12 else 1, 2 if self.depth == 10 else 1
        ptrs = np.array([self.y.data_ptr(), self.u.data_ptr(), self.u.data_ptr() + size if self.nv12 else self.v.data_ptr()], dtype=np.uint64)
        nums = [Ts, Hs, Ws, int(Wr), _plane_stride(self.y, 1, Ws) * size, _plane_stride(self.y, 0, 0) * size,
                _plane_stride(self.u, 1, (Ws + 1) // 2 * step) * size, _plane_stride(self.u, 0, 0) * size, step, self.depth,
                self.shift] + list(self.matrix) + [0]
        return np.concatenate([ptrs.view(np.int32), np.array(nums, dtype=np.int32)])

    def __repr__(self):
        if getattr(self, 'depth', 8) == 10:
            return (f'YUVClip({"P010" if self.nv12 else "yuv420p10"} {"msb" if self.shift else "lsb"}-aligned {self.shape} on {self.device}, '
                    f'matrix={self.matrix})')
        return f'YUVClip({"NV12" if self.nv12 else "I420"} {self.shape} on {self.device}, matrix={self.matrix})'


def clip_dims(clip):
    """(B, T, C, H, W) of a float [B,T,C,H,W] or a uint8 channels-last [B,T,H,W,3] clip (or the MixedClip of one)."""
    if clip.dtype == torch.uint8:
        B, T, H, W, Cc = clip.shape
        if Cc != 3:
            raise ValueError('uint8 clips must be [B,T,H,W,3]')
        return B, T, Cc, H, W
    B, T, Cc, H, W = clip.shape
    return B, T, Cc, H, W


def patch_rows(clip, dtype, ps, ts, frame_major):
    """[B,T,C,H,W] fp32 -> [B*(T/ts)*P, C*ts*ps*ps] rows in `dtype`; a uint8 [B,T,H,W,3] clip is
    normalised on the fly (ToTensor + Normalize of the reference, see set_input_normalization), and the
    MixedClip of one is normalised and mixed on the fly."""
    need_cuda(clip)
    if isinstance(clip, MixedClip):
        import numpy as np
        if _input_norm is None:
            raise ValueError('MixedClip: call vtx.set_input_normalization(mean, std) first')
        B, T, Cc, H, W = clip_dims(clip)
        K = Cc * ts * ps * ps
        rows = torch.empty(B * (T // ts) * (H // ps) * (W // ps), K, dtype=dtype, device=clip.device)
        mean = (C.c_float * 3)(*_input_norm[0])
        std = (C.c_float * 3)(*_input_norm[1])
        with _timed('patch_rows', nbytes=clip.clip.numel() + rows.numel() * rows.element_size(), key=f'mix u8 {B}x{T}'):
            # lam and 1 - lam as mixup_batch_ hands them over: 1 - lam in float64, each rounded once
            _lib.mix_call('vtx_patch_rows_mix_u8', _DT[dtype], B, T, H, W, ps, ts, ptr(clip.clip), mean, std,
                          float(np.float32(clip.lam)), float(np.float32(1. - clip.lam)), ptr(rows), K, int(frame_major), stream())
        return rows
    if clip.dtype == torch.uint8:
        if _input_norm is None:
            raise ValueError('uint8 clip: call vtx.set_input_normalization(mean, std) first')
        clip = clip.contiguous()
        B, T, Cc, H, W = clip_dims(clip)
        K = Cc * ts * ps * ps
        rows = torch.empty(B * (T // ts) * (H // ps) * (W // ps), K, dtype=dtype, device=clip.device)
        mean = (C.c_float * 3)(*_input_norm[0])
        std = (C.c_float * 3)(*_input_norm[1])
        with _timed('patch_rows', nbytes=clip.numel() + rows.numel() * rows.element_size(), key=f'u8 {B}x{T}'):
            call('vtx_patch_rows_u8', _DT[dtype], B, T, H, W, ps, ts, ptr(clip), mean, std, ptr(rows), K, int(frame_major),
                 stream())
        return rows
    if clip.dtype != torch.float32:
        clip = clip.float()
    clip = clip.contiguous()
    B, T, Cc, H, W = clip.shape
    K = Cc * ts * ps * ps
    rows = torch.empty(B * (T // ts) * (H // ps) * (W // ps), K, dtype=dtype, device=clip.device)
    with _timed('patch_rows', nbytes=clip.numel() * 4 + rows.numel() * rows.element_size(), key=f'f32 {B}x{T}'):
        call('vtx_patch_rows', _DT[dtype], B, T, Cc, H, W, ps, ts, ptr(clip), ptr(rows), K, int(frame_major), stream())
    return rows


def _u8_clip(clip, who):
    """The checks every uint8-clip entry makes, shape first (reachable without a device): contiguous uint8 CUDA [B,T,H,W,3]."""
    if not isinstance(clip, torch.Tensor) or clip.dtype != torch.uint8:
        raise TypeError(f'{who}: a uint8 tensor is required, got {getattr(clip, "dtype", type(clip).__name__)}')
    if clip.ndim != 5 or clip.shape[-1] != 3:
        raise ValueError(f'{who}: the uint8 clip must be [B,T,H,W,3] (channels last), got {tuple(clip.shape)}')
    need_cuda(clip)
    return clip.contiguous()


def im2col3d_u8(clip, k3, s3, p3, Kp, dtype):
    """uint8 [B,T,H,W,3] -> the rows [B*To*Ho*Wo, Kp] (`dtype`) of an overlapping, padded Conv3d on the normalised clip (ToTensor +
    Normalize of the reference on the fly, see set_input_normalization; padding taps and the columns behind 3*kt*kh*kw are
    +0): bit for bit the rows vtx_im2col3d makes of the normalised float [B,T,3,H,W] clip (vtx_im2col3d_u8, libvtx_stem.so)."""
    clip = _u8_clip(clip, 'im2col3d_u8')
    if _input_norm is None:
        raise ValueError('uint8 clip: call vtx.set_input_normalization(mean, std) first')
    B, T, H, W, _ = clip.shape
    k3, s3, p3 = ([int(v) for v in t] for t in (k3, s3, p3))
    if len(k3) != 3 or len(s3) != 3 or len(p3) != 3:
        raise ValueError('im2col3d_u8: k3, s3, p3 are (t, h, w) triples')
    To, Ho, Wo = ((n + 2 * p - k) // s + 1 if s > 0 else 0 for n, p, k, s in zip((T, H, W), p3, k3, s3))
    rows = torch.empty(max(B * To * Ho * Wo, 0), int(Kp), dtype=dtype, device=clip.device)
    i3 = lambda t: (C.c_int * 3)(*t)   # noqa: E731
    mean = (C.c_float * 3)(*_input_norm[0])
    std = (C.c_float * 3)(*_input_norm[1])
    with _timed('im2col3d', nbytes=clip.numel() + rows.numel() * rows.element_size(), key=f'u8 {B}x{T}'):
        _lib.stem_call('vtx_im2col3d_u8', _DT[dtype], B, T, H, W, i3(k3), i3(s3), i3(p3), int(Kp), ptr(clip), mean, std, ptr(rows),
                       stream())
    return rows


def embed_table(dtype, P, T, D, bias, pos, time_embed, cls, frame_major=False):
    dev = pos.device
    E = torch.empty(P * T, D, dtype=dtype, device=dev)
    cls_row = torch.empty(D, dtype=dtype, device=dev) if cls is not None else None
    call('vtx_embed_table', _DT[dtype], P, T, D, ptr(bias), ptr(pos), ptr(time_embed), ptr(cls), ptr(E),
         ptr(cls_row), int(frame_major), stream())
    return E, cls_row


# ------------------------------------------------------------------------ HOG
_hog_tables = {}


def hog_table(device):
    key = str(device)
    if key not in _hog_tables:
        host = torch.empty(_lib.load().vtx_hog_table_bytes() // 8, dtype=torch.float64)     # magnitudes + the correction words
        call('vtx_hog_build_table', host.data_ptr())
        _hog_tables[key] = host.to(device)
    return _hog_tables[key]


def hog_fwd(frames, want_bins=False):
    """frames uint8 [F,H,W,3] (CUDA) -> float64 [F,H/16,W/16,108] (+ int32 bins [F,3,H,W])."""
    need_cuda(frames)
    if frames.dtype != torch.uint8 or frames.ndim != 4 or frames.shape[-1] != 3:
        raise TypeError('hog_fwd: frames must be uint8 [F,H,W,3]')
    frames = frames.contiguous()
    F, H, W, _ = frames.shape
    out = torch.empty(F, H // 16, W // 16, 108, dtype=torch.float64, device=frames.device)
    bins = torch.empty(F, 3, H, W, dtype=torch.int32, device=frames.device) if want_bins else None
    table = hog_table(frames.device)
    with _timed('hog', nbytes=frames.numel() + out.numel() * 8, key=f'{F}x{H}x{W}'):
        call('vtx_hog_fwd', ptr(frames), F, H, W, ptr(table), table.numel() * 8, ptr(out), ptr(bins), stream())
    return (out, bins) if want_bins else out


def hog_center_frames(cube_marker, num_frames, tstride=2):
    """The flat frame indices b*T + centre of the centre frames of a batch's masked cubes, sorted, each once: the centre of
    marker [start, span] is start*tstride + span*tstride//2, the expression of video_transformer.center_frame_mask (reference
    video_transformer.py:889-896).  A clip with no marker contributes none; a centre outside 0 .. T-1 raises ValueError."""
    T, ts = int(num_frames), int(tstride)
    sel = set()
    for b, markers in enumerate(cube_marker):
        for start, span in markers:
            c = int(start) * ts + int(span) * ts // 2
            if not 0 <= c < T:
                raise ValueError(f'hog_targets: marker [{int(start)}, {int(span)}] of clip {b} has its centre frame {c} outside 0..{T - 1}')
            sel.add(b * T + c)
    return sorted(sel)


def hog_targets(clip, cube_marker, tstride=2):
    """MaskFeat's regression targets from the decoded clip (reference dataset.py:188-196: HOG of the centre frame of every masked
    cube, computed there on CPU workers): uint8 [B,T,H,W,3] (CUDA) + cube_marker (per clip a list of [start, span]) -> float64
    [B,T,H/16,W/16,108], zeros outside the centre frames.  One index upload and one launch for the batch (vtx_hog_fwd_sel,
    libvtx_stem.so); each selected frame equals hog_fwd of that frame bit for bit."""
    clip = _u8_clip(clip, 'hog_targets')
    B, T, H, W, _ = clip.shape
    if len(cube_marker) != B:
        raise ValueError(f'hog_targets: {len(cube_marker)} marker lists for {B} clips')
    if H <= 0 or W <= 0 or H % 16 or W % 16 or W > 1024:
        raise ValueError(f'hog_targets: H={H}, W={W} must be multiples of 16 (W <= 1024)')
    sel = hog_center_frames(cube_marker, T, tstride)
    out = torch.zeros(B, T, H // 16, W // 16, 108, dtype=torch.float64, device=clip.device)
    if not sel:
        return out
    table = hog_table(clip.device)
    idx = upload_i32(sel, clip.device)
    with _timed('hog', nbytes=len(sel) * (H * W * 3 + out[0, 0].numel() * 8), key=f'sel {len(sel)}x{H}x{W}'):
        _lib.stem_call('vtx_hog_fwd_sel', ptr(clip), B * T, H, W, ptr(idx), len(sel), ptr(table), table.numel() * 8, ptr(out), stream())
    return out


# ------------------------------------------------- clip augmentation (csrc/aug.hip -> libvtx_aug.so)
RESAMPLE_MODES = {'bilinear': _lib.RESAMPLE_BILINEAR, 'bicubic': _lib.RESAMPLE_BICUBIC}


def _resample_mode(mode):
    try:
        return RESAMPLE_MODES[mode]
    except KeyError:
        raise ValueError(f"resample: interpolation {mode!r} is not built ('bilinear' or 'bicubic')")


def resample_max_taps(crop_len, out_len, mode, antialias=False):
    """Taps per output index a table of vtx_resample_build_table needs (host only)."""
    n = _lib.load_aug().vtx_resample_max_taps(int(crop_len), int(out_len), _resample_mode(mode), int(bool(antialias)))
    if n <= 0:
        _lib.aug_check(n, 'vtx_resample_max_taps')
    return n


def resample_table(src_len, crop_start, crop_len, out_len, mode, antialias=False, flip=False, max_taps=None):
    """F.interpolate(align_corners=False) weights of one axis (host only, NumPy): first int32 [out_len], count int32 [out_len],
    weights float32 [out_len, max_taps] (zero behind ``count``)."""
    import numpy as np
    if max_taps is None:
        max_taps = resample_max_taps(crop_len, out_len, mode, antialias)
    first = np.zeros(out_len, dtype=np.int32)
    count = np.zeros(out_len, dtype=np.int32)
    weights = np.zeros((out_len, max_taps), dtype=np.float32)
    _lib.aug_call('vtx_resample_build_table', int(src_len), int(crop_start), int(crop_len), int(out_len), _resample_mode(mode),
         int(bool(antialias)), int(bool(flip)), int(max_taps), first.ctypes.data, count.ctypes.data, weights.ctypes.data)
    return first, count, weights


def _check_u8_clip(clip, what):
    need_cuda(clip)
    if clip.dtype != torch.uint8 or clip.ndim != 5 or clip.shape[-1] != 3:
        raise TypeError(f'{what}: clip must be uint8 [B,T,H,W,3], got {clip.dtype} {tuple(clip.shape)}')


def _is_table(tab, B, n=None):
    """Is ``tab`` a resample table of B clips and n outputs (None: as many as it holds): (first int32 [B,n], count int32 [B,n],
    weights float32 [B,n,taps]), contiguous device tensors?"""
    f, c, w = tab
    need_cuda(f, c, w)
    if n is None:
        n = f.shape[1] if f.ndim == 2 else -1
    return (f.dtype == torch.int32 and c.dtype == torch.int32 and w.dtype == torch.float32 and tuple(f.shape) == (B, n)
            and tuple(c.shape) == (B, n) and w.ndim == 3 and tuple(w.shape[:2]) == (B, n)
            and f.is_contiguous() and c.is_contiguous() and w.is_contiguous())


def _table_lengths(name, B, xtab, ytab):
    """The tables of the view kernels, whose output lengths the tables themselves give -> (columns of xtab, rows of ytab)."""
    for tab in (xtab, ytab):
        if not _is_table(tab, B) or tab[0].shape[1] < 1 or tab[2].shape[2] < 1:
            raise TypeError(f'{name}: a table is (int32 [{B},n], int32 [{B},n], float32 [{B},n,taps]), contiguous')
    return xtab[0].shape[1], ytab[0].shape[1]


def clip_resample_u8(src, out_hw, xtab, ytab):
    """src uint8 [B,T,Hs,Ws,3] -> uint8 [B,T,H,W,3].  xtab = (first [B,W] int32, count [B,W] int32, weights [B,W,K] float32)
    device tensors, one resample_table per clip; ytab likewise with H."""
    _check_u8_clip(src, 'clip_resample_u8')
    src = src.contiguous()
    B, T, Hs, Ws, _ = src.shape
    H, W = int(out_hw[0]), int(out_hw[1])
    for tab, n in ((xtab, W), (ytab, H)):
        if not _is_table(tab, B, n):
            raise TypeError(f'clip_resample_u8: a table is (int32 [{B},{n}], int32 [{B},{n}], float32 [{B},{n},taps]), contiguous')
    dst = torch.empty(B, T, H, W, 3, dtype=torch.uint8, device=src.device)
    with _timed('clip_resample', nbytes=src.numel() + dst.numel(), key=f'{B}x{T} {Hs}x{Ws}->{H}x{W}'):
        _lib.aug_call('vtx_clip_resample_u8', B, T, Hs, Ws, H, W, ptr(src), ptr(dst), ptr(xtab[0]), ptr(xtab[1]), ptr(xtab[2]),
             xtab[2].shape[2], ptr(ytab[0]), ptr(ytab[1]), ptr(ytab[2]), ytab[2].shape[2], stream())
    return dst


def clip_jitter_u8_(clip, jit_ops, factors):
    """In place on a contiguous uint8 [B,T,H,W,3] clip: per clip, jit_ops [B,4] int32 = {n, op, op, op} (0 brightness, 1 contrast,
    2 saturation) applied in that order with factors [B,6] float32 = {r, r, r, 1 - r, 1 - r, 1 - r} (torchvision's ColorJitter
    without hue; 1 - r is formed in float64 and rounded on its own, as torchvision's _blend does)."""
    _check_u8_clip(clip, 'clip_jitter_u8_')
    need_cuda(jit_ops, factors)
    B, T, H, W, _ = clip.shape
    if not clip.is_contiguous():
        raise TypeError('clip_jitter_u8_: contiguous clip required (in place)')
    if (jit_ops.dtype != torch.int32 or tuple(jit_ops.shape) != (B, 4) or factors.dtype != torch.float32
            or tuple(factors.shape) != (B, 6) or not (jit_ops.is_contiguous() and factors.is_contiguous())):
        raise TypeError(f'clip_jitter_u8_: jit_ops int32 [{B},4] and factors float32 [{B},6], contiguous')
    ws = torch.empty(_lib.load_aug().vtx_clip_jitter_workspace(B, T) // 4, dtype=torch.int32, device=clip.device)
    with _timed('clip_jitter', nbytes=3 * clip.numel(), key=f'{B}x{T} {H}x{W}'):
        _lib.aug_call('vtx_clip_jitter_u8', B, T, H, W, ptr(clip), ptr(jit_ops), ptr(factors), ptr(ws), ws.numel() * 4, stream())
    return clip


# ------------------------------------------------- RandAugment (csrc/randaug.hip -> libvtx_randaug.so)
def _check_record(t, B, n, dtype, what):
    need_cuda(t)
    if t.dtype != dtype or tuple(t.shape) != ((B, n) if n else (B,)) or not t.is_contiguous():
        raise TypeError(f'{what}: {str(dtype).replace("torch.", "")} [{B}{f",{n}" if n else ""}] contiguous device tensor expected, '
                        f'got {t.dtype} {tuple(t.shape)}')


def _randaug_out_of_place(name, cls, src, rec, rec_n, sel, out, nbytes_per):
    _check_u8_clip(src, name)
    B, T, H, W, _ = src.shape
    _check_record(rec, B, rec_n, torch.float32, name)
    _check_record(sel, B, 0, torch.int32, name)
    if not src.is_contiguous():
        raise TypeError(f'{name}: contiguous clip required')
    if out is None:
        out = torch.empty_like(src)
    else:
        _check_u8_clip(out, name)
        if out is src or out.data_ptr() == src.data_ptr():
            raise ValueError(f'{name}: out of place only (out is the source clip)')
        if out.shape != src.shape or not out.is_contiguous():
            raise TypeError(f'{name}: out must be a contiguous uint8 {tuple(src.shape)} clip')
    with _timed(cls, nbytes=nbytes_per * src.numel(), key=f'{B}x{T} {H}x{W}'):
        _lib.randaug_call('vtx_' + name, B, T, H, W, ptr(src), ptr(out), ptr(rec), ptr(sel), stream())
    return out


def clip_warp_nearest_u8(src, theta, sel, out=None):
    """uint8 [B,T,H,W,3] -> a new clip (or ``out``): the nearest-neighbour affine warp of RandAugment's ShearX/Y, TranslateX/Y and
    Rotate.  theta float32 [B,6]: the inverse matrix of torchvision's _get_inverse_affine_matrix; sel int32 [B]: 0 = copy the clip."""
    return _randaug_out_of_place('clip_warp_nearest_u8', 'clip_warp', src, theta, 6, sel, out, 2)


def clip_sharpness_u8(src, factors, sel, out=None):
    """uint8 [B,T,H,W,3] -> a new clip (or ``out``): torchvision's adjust_sharpness.  factors float32 [B,2] = {r, 1 - r} (1.0 - r
    formed in float64 and rounded on its own); sel int32 [B]: 0 = copy the clip."""
    return _randaug_out_of_place('clip_sharpness_u8', 'clip_sharpness', src, factors, 2, sel, out, 2)


def _in_place_clip(clip, what):
    _check_u8_clip(clip, what)
    if not clip.is_contiguous():
        raise TypeError(f'{what}: contiguous clip required (in place)')
    return clip.shape[:4]


def clip_pointwise_u8_(clip, pw_ops):
    """In place: pw_ops int32 [B,2] = {0 none | 1 posterize | 2 solarize, argument} (bits to keep | integer threshold)."""
    B, T, H, W = _in_place_clip(clip, 'clip_pointwise_u8_')
    _check_record(pw_ops, B, 2, torch.int32, 'clip_pointwise_u8_')
    with _timed('clip_pointwise', nbytes=2 * clip.numel(), key=f'{B}x{T} {H}x{W}'):
        _lib.randaug_call('vtx_clip_pointwise_u8', B, T, H, W, ptr(clip), ptr(pw_ops), stream())
    return clip


def _randaug_two_pass(name, cls, clip, sel):
    B, T, H, W = _in_place_clip(clip, name + '_')
    _check_record(sel, B, 0, torch.int32, name + '_')
    lib = _lib.load_randaug()
    nbytes = getattr(lib, f'vtx_{name[:-3]}_workspace')(B, T)
    ws = torch.empty(nbytes // 4, dtype=torch.int32, device=clip.device)
    with _timed(cls, nbytes=3 * clip.numel(), key=f'{B}x{T} {H}x{W}'):
        _lib.randaug_call(f'vtx_{name}', B, T, H, W, ptr(clip), ptr(sel), ptr(ws), nbytes, stream())
    return clip


def clip_autocontrast_u8_(clip, sel):
    """In place: torchvision's autocontrast per frame and channel on the clips with sel[b] != 0 (sel int32 [B])."""
    return _randaug_two_pass('clip_autocontrast_u8', 'clip_autocontrast', clip, sel)


def clip_equalize_u8_(clip, sel):
    """In place: torchvision's equalize per frame and channel on the clips with sel[b] != 0 (sel int32 [B])."""
    return _randaug_two_pass('clip_equalize_u8', 'clip_equalize', clip, sel)


# ------------------------------------------------- test-time views (csrc/views.hip -> libvtx_views.so)
def _index_rows(name, t, B, what):
    """frames / left of the view kernels, [B,n]: an int32 device tensor is returned as it is (the kernel clamps what it reads;
    whoever built it validated it); host values -- a CPU integer tensor, an array or nested lists -- come back as an integer
    array whose range the caller checks."""
    import numpy as np
    if isinstance(t, torch.Tensor) and t.is_cuda:
        need_cuda(t)
        if t.dtype != torch.int32 or t.ndim != 2 or t.shape[0] != B or t.shape[1] < 1 or not t.is_contiguous():
            raise TypeError(f'{name}: {what} must be int32 [{B},n] contiguous, got {t.dtype} {tuple(t.shape)}')
        return t
    a = t.numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    if a.dtype.kind not in 'iu' or a.ndim != 2 or a.shape[0] != B or a.shape[1] < 1:
        raise TypeError(f'{name}: {what} must be integers [{B},n], got {a.dtype} {a.shape}')
    return a


def _views_index(t, B, lo, hi, what, device):
    """frames / left of clip_views_u8: host values are checked against lo <= v <= hi and uploaded."""
    a = _index_rows('clip_views_u8', t, B, what)
    if isinstance(a, torch.Tensor):
        return a
    if a.min() < lo or a.max() > hi:
        raise ValueError(f'clip_views_u8: {what} must lie in {lo} .. {hi}, got {int(a.min())} .. {int(a.max())}')
    return upload_i32(a, device).view(a.shape)


def clip_views_u8(src, frames, left, width, xtab, ytab, out=None):
    """Frame selection, resize and V crops of ``width`` columns in one launch: src uint8 [B,Ts,Hs,Ws,3] -> uint8 [B,V,T,H,width,3],
    view v of clip b = columns left[b,v] .. left[b,v] + width of the resized frames src[b, frames[b]].  frames: [B,T] indices into
    Ts, or None for every frame; left: [B,V], V <= 8 (both: int32 device tensors, or host integers, which are validated and
    uploaded).  xtab = (first [B,Wr] int32, count [B,Wr] int32, weights [B,Wr,K] float32) device tensors for ALL columns of the
    resized frame, ytab likewise for the H output rows.  Byte for byte clip_resample_u8 on the gathered frames, sliced.
    ``out``: a contiguous uint8 [B,V,T,H,width,3] device tensor to write into."""
    _check_u8_clip(src, 'clip_views_u8')
    src = src.contiguous()
    B, Ts, Hs, Ws, _ = src.shape
    W = int(width)
    Wr, H = _table_lengths('clip_views_u8', B, xtab, ytab)
    if not 0 < W <= Wr:
        raise ValueError(f'clip_views_u8: views of {W} columns do not fit the resized row of {Wr}')
    left = _views_index(left, B, 0, Wr - W, f'left (left + width <= {Wr})', src.device)
    V = left.shape[1]
    if V > _lib.VIEWS_MAX:
        raise ValueError(f'clip_views_u8: {V} views, at most {_lib.VIEWS_MAX}')
    if frames is None:
        T = Ts
    else:
        frames = _views_index(frames, B, 0, Ts - 1, f'frame indices into {Ts} frames', src.device)
        T = frames.shape[1]
    if out is None:
        out = torch.empty(B, V, T, H, W, 3, dtype=torch.uint8, device=src.device)
    else:
        need_cuda(out)
        if out.dtype != torch.uint8 or tuple(out.shape) != (B, V, T, H, W, 3) or not out.is_contiguous():
            raise TypeError(f'clip_views_u8: out must be a contiguous uint8 {(B, V, T, H, W, 3)} tensor, got {out.dtype} {tuple(out.shape)}')
    with _timed('clip_views', nbytes=B * T * Hs * Ws * 3 + out.numel(), key=f'{B}x{T}/{Ts} {Hs}x{Ws}->{V}x{H}x{W}'):
        _lib.views_call('vtx_clip_views_u8', B, Ts, T, Hs, Ws, H, Wr, V, W, ptr(src), ptr(out), ptr(frames), ptr(left),
                        ptr(xtab[0]), ptr(xtab[1]), ptr(xtab[2]), xtab[2].shape[2], ptr(ytab[0]), ptr(ytab[1]), ptr(ytab[2]),
                        ytab[2].shape[2], stream())
    return out


# ------------------------------------------------- views of clips that differ in source size (csrc/ragged.hip -> libvtx_ragged.so)
def clip_list_shapes(clips, what):
    """A ragged batch: a non-empty list or tuple of uint8 [Ts_b,Hs_b,Ws_b,3] tensors -> [(Ts_b, Hs_b, Ws_b)].  Types and shapes
    only (host); where the tensors live is ``clips_table``'s check."""
    if not isinstance(clips, (list, tuple)):
        raise TypeError(f'{what}: a list or tuple of uint8 [T,H,W,3] clips expected, got {type(clips).__name__}')
    if len(clips) == 0:
        raise ValueError(f'{what}: an empty list of clips')
    if any(isinstance(c, YUVClip) for c in clips):               # a list of 4:2:0 clips (clips_views_yuv): all of them are
        for b, c in enumerate(clips):
            if not isinstance(c, YUVClip):
                raise TypeError(f'{what}: clip {b} is a {type(c).__name__} beside YUVClip entries: a list holds tensors or YUVClip, not both')
        return [c.shape for c in clips]
    for b, c in enumerate(clips):
        if not isinstance(c, torch.Tensor):
            raise TypeError(f'{what}: clip {b} is a {type(c).__name__}, not a tensor')
        if c.dtype != torch.uint8 or c.ndim != 4 or c.shape[-1] != 3 or c.numel() == 0:
            raise TypeError(f'{what}: clip {b} must be a non-empty uint8 [T,H,W,3], got {c.dtype} {tuple(c.shape)}')
    return [tuple(c.shape[:3]) for c in clips]


class ClipTable:
    """A list of clips that passed every host check, and the descriptor vtx_clips_views_u8 reads on the device.  ``kept``: the
    clips made contiguous (referenced here until the launch is enqueued); ``shapes``: [(Ts_b, Hs_b, Ws_b)]; ``widths``: the columns
    of each clip's resized row; ``host``: int32 array [6 * B] -- the B base pointers as little-endian int32 pairs, then B records
    (Ts_b, Hs_b, Ws_b, widths[b]).  The pointers come FIRST: whoever packs ``host`` into a larger upload puts it at the front,
    where the 8-byte loads of the pointers are aligned.  Only ``clips_table`` makes one.

    Of a list of ``YUVClip`` (``yuv`` is then True): ``kept`` holds the carriers, whose planes are read in place, and ``host`` is
    int32 [22 * B], the B records vtx_clips_views_yuv420 reads (include/vtx_yuv.h: each begins with its three pointers).  With
    at least one 10-bit clip in the list ``deep`` is True and ``host`` is int32 [24 * B], the records of every clip, 8-bit ones
    included, as vtx_clips_views_yuv10 reads them (include/vtx_yuv10.h)."""
    __slots__ = ('kept', 'shapes', 'widths', 'host', 'yuv', 'deep')

    @property
    def device(self):
        return self.kept[0].device


def clips_table(clips, widths, what='clips_views_u8'):
    """list or tuple of uint8 CUDA clips [Ts_b,Hs_b,Ws_b,3] on the current device -- or of YUVClip --, B row widths -> ClipTable.
    Host only: nothing is enqueued but the copies of entries that are not contiguous."""
    import numpy as np
    t = ClipTable()
    t.shapes = clip_list_shapes(clips, what)
    t.yuv = isinstance(clips[0], YUVClip)
    t.deep = t.yuv and any(c.depth == 10 for c in clips)
    need_cuda(*([p for c in clips for p in c.planes] if t.yuv else clips))
    t.widths = [int(w) for w in widths]
    if len(t.widths) != len(clips):
        raise ValueError(f'{what}: {len(t.widths)} row widths for {len(clips)} clips')
    if t.yuv:
        t.kept = list(clips)
        t.host = np.concatenate([c.record10(w) if t.deep else c.record(w) for c, w in zip(clips, t.widths)])
        return t
    t.kept = [c.contiguous() for c in clips]
    ptrs = np.array([c.data_ptr() for c in t.kept], dtype=np.uint64)
    geom = np.array([s + (w,) for s, w in zip(t.shapes, t.widths)], dtype=np.int32)
    t.host = np.concatenate([ptrs.view(np.int32), geom.reshape(-1)])
    return t


def _ragged_index(t, B, hi, what, device, name='clips_views_u8'):
    """frames / left of clips_views_u8: host integers are checked row by row against 0 <= v <= hi[b] (the clip's own numbers)
    -> int32 array [B,n], not yet uploaded."""
    import numpy as np
    a = _index_rows(name, t, B, what)
    if isinstance(a, torch.Tensor):
        return a
    bad = ((a < 0) | (a > np.asarray(hi).reshape(B, 1))).any(axis=1)
    if bad.any():
        b = int(np.argmax(bad))
        raise ValueError(f'{name}: {what} of clip {b} must lie in 0 .. {hi[b]}, got {int(a[b].min())} .. {int(a[b].max())}')
    return np.ascontiguousarray(a, dtype=np.int32)


def clips_views_u8(clips, frames, left, width, xtab, ytab, out=None, widths=None, table=None):
    """clip_views_u8 for clips that differ in decoded length and frame size, in one launch: ``clips`` a list or tuple of B uint8
    CUDA tensors [Ts_b,Hs_b,Ws_b,3] on the current device -> uint8 [B,V,T,H,width,3].  frames: [B,T] indices, row b into the Ts_b
    frames of its own clip, or None for every frame (all Ts_b must then be equal); left: [B,V], V <= 8, first columns in clip b's
    resized row of widths[b] columns (both: int32 device tensors, or host integers, which are validated and uploaded).  xtab =
    (first [B,Wr_max] int32, count [B,Wr_max] int32, weights [B,Wr_max,K] float32) device tensors, row b valid for its first
    widths[b] columns (``widths``: B integers in width .. Wr_max; None = Wr_max for every clip); ytab likewise for the H output
    rows.  Clip b's views are byte for byte clip_views_u8 on clips[b][None] with row b of the tables.

    Entries that are not contiguous are copied; the copies live until the launch is enqueued.  Everything is checked on the host
    before anything is enqueued, and the pointer table is built only from tensors that passed.  It is uploaded, with the
    geometry and whatever of frames / left came as host values, in one copy.  A caller with records of its own to upload
    (vtx.aug: tables, colour records and descriptor in one copy) passes the ``ClipTable`` of ``clips_table`` as ``clips`` and
    the int32 [6 * B] device copy of its ``host`` array as ``table``; the list is then not checked again."""
    return _clips_views('clips_views_u8', False, clips, frames, left, width, xtab, ytab, out, widths, table)


def _clips_views(name, yuv, clips, frames, left, width, xtab, ytab, out, widths, table):
    """clips_views_u8 (yuv False: tensors, vtx_clips_views_u8) and clips_views_yuv (yuv True: YUVClip, vtx_clips_views_yuv420, or
    vtx_clips_views_yuv10 for a list with a 10-bit clip in it): the same checks, the same upload and the same arguments behind
    the descriptor."""
    import numpy as np
    if isinstance(clips, ClipTable):
        ct = clips
        if widths is not None:
            raise TypeError(f'{name}: a ClipTable carries its row widths')
    else:
        if table is not None:
            raise TypeError(f'{name}: table= goes with the ClipTable it is the device copy of')
        shapes = clip_list_shapes(clips, name)                   # types and shapes before the tables' batch size is read
        ct = None
    if isinstance((ct.kept if ct else clips)[0], YUVClip) != yuv:
        raise TypeError(f'{name}: a list of ' + ('YUVClip is expected, got tensors (clips_views_u8 takes those)' if yuv else
                                                 'uint8 tensors is expected, got YUVClip (clips_views_yuv takes those)'))
    if ct is None:
        need_cuda(*([p for c in clips for p in c.planes] if yuv else clips))
    B, W = len(ct.kept if ct else clips), int(width)
    Wr_max, H = _table_lengths(name, B, xtab, ytab)
    if ct is None:
        ct = clips_table(clips, [Wr_max] * B if widths is None else widths, name)
    shapes, widths, dev = ct.shapes, ct.widths, ct.device
    words = (_lib.YUV10_CLIP_I32 if ct.deep else _lib.YUV_CLIP_I32) if yuv else 6       # int32 words of the descriptor per clip
    for b, w in enumerate(widths):
        if not 0 < W <= w <= Wr_max:
            raise ValueError(f'{name}: views of {W} columns do not fit the resized row of {w} of clip {b} (the tables hold {Wr_max})')
    left = _ragged_index(left, B, [w - W for w in widths], 'left (left + width <= the row of the clip)', dev, name)
    V = left.shape[1]
    if V > _lib.VIEWS_MAX:
        raise ValueError(f'{name}: {V} views, at most {_lib.VIEWS_MAX}')
    if frames is None:
        T = shapes[0][0]
        if any(s[0] != T for s in shapes):
            raise ValueError(f'{name}: without frame indices every frame is taken and the clips must agree in length, got {[s[0] for s in shapes]}')
    else:
        frames = _ragged_index(frames, B, [s[0] - 1 for s in shapes], 'frame indices (into the frames of the clip)', dev, name)
        T = frames.shape[1]
    if B * T > 65535:
        raise ValueError(f'{name}: {B} clips x {T} frames exceed the grid (65535)')
    if out is None:
        out = torch.empty(B, V, T, H, W, 3, dtype=torch.uint8, device=dev)
    else:
        need_cuda(out)
        if out.dtype != torch.uint8 or tuple(out.shape) != (B, V, T, H, W, 3) or not out.is_contiguous():
            raise TypeError(f'{name}: out must be a contiguous uint8 {(B, V, T, H, W, 3)} tensor, got {out.dtype} {tuple(out.shape)}')
    if table is None:
        parts = [ct.host] + [a.reshape(-1) for a in (left, frames) if isinstance(a, np.ndarray)]
        up = upload_i32(np.concatenate(parts), dev)
        table, at = up[:words * B], words * B
        if isinstance(left, np.ndarray):
            left, at = up[at:at + left.size].view(left.shape), at + left.size
        if isinstance(frames, np.ndarray):
            frames = up[at:at + frames.size].view(frames.shape)
    else:
        need_cuda(table)
        if (table.dtype != torch.int32 or table.ndim != 1 or table.numel() != words * B or not table.is_contiguous()
                or table.data_ptr() % 8):
            raise TypeError(f'{name}: table must be the int32 [{words * B}] device copy of the ClipTable\'s host array, 8-byte aligned')
        if isinstance(left, np.ndarray) or isinstance(frames, np.ndarray):
            raise TypeError(f'{name}: with table= frames and left are device tensors (uploaded with it)')
    tabs = (ptr(frames), ptr(left), ptr(xtab[0]), ptr(xtab[1]), ptr(xtab[2]), xtab[2].shape[2], ptr(ytab[0]), ptr(ytab[1]), ptr(ytab[2]),
            ytab[2].shape[2], stream())
    if yuv and ct.deep:                                          # one launch for both depths: 1.5 samples per pixel of 1 or 2 bytes
        src_bytes = sum(T * c.source_bytes for c in ct.kept)
        with _timed('clips_views_yuv10', nbytes=src_bytes + out.numel(), key=f'{B}x{T} yuv420p10->{V}x{H}x{W}'):
            _lib.yuv10_call('vtx_clips_views_yuv10', B, T, H, V, W, Wr_max, ptr(table), ptr(out), *tabs)
        return out
    if yuv:                                                      # 1.5 source bytes per pixel: the luma and two quarter-size chroma planes
        src_bytes = sum(T * (s[1] * s[2] + 2 * ((s[1] + 1) // 2) * ((s[2] + 1) // 2)) for s in shapes)
        with _timed('clips_views_yuv', nbytes=src_bytes + out.numel(), key=f'{B}x{T} yuv420->{V}x{H}x{W}'):
            _lib.yuv_call('vtx_clips_views_yuv420', B, T, H, V, W, Wr_max, ptr(table), ptr(out), *tabs)
        return out
    src_bytes = sum(T * s[1] * s[2] * 3 for s in shapes)
    with _timed('clips_views', nbytes=src_bytes + out.numel(), key=f'{B}x{T} ragged->{V}x{H}x{W}'):
        _lib.ragged_call('vtx_clips_views_u8', B, T, H, V, W, Wr_max, ptr(table), table.data_ptr() + 8 * B, ptr(out), ptr(frames),
                         ptr(left), ptr(xtab[0]), ptr(xtab[1]), ptr(xtab[2]), xtab[2].shape[2], ptr(ytab[0]), ptr(ytab[1]),
                         ptr(ytab[2]), ytab[2].shape[2], stream())
    return out                                                   # (ct.kept lived until here: the launch is enqueued)


# ------------------------------------------------- 4:2:0 YUV clips into the resampler (csrc/yuv.hip -> libvtx_yuv.so)
def clips_views_yuv(clips, frames, left, width, xtab, ytab, out=None, widths=None, table=None):
    """clips_views_u8 on decoded 4:2:0 clips: ``clips`` a list or tuple of B ``YUVClip`` (NV12 and I420, sizes, pitches and
    matrices may differ from clip to clip) -> uint8 [B,V,T,H,width,3], byte for byte clips_views_u8 on the clips
    ``yuv420_to_rgb_u8`` would write, which never exist: each tap is converted in registers.  Every other argument, every check
    and the one upload are clips_views_u8's; ``table``: the int32 [22 * B] device copy of the ClipTable's ``host`` array.

    A list whose clips are all 8-bit launches vtx_clips_views_yuv420 (libvtx_yuv.so).  A list with at least one 10-bit clip
    (P010, yuv420p10le: ``YUVClip(depth=10)``) launches vtx_clips_views_yuv10 (libvtx_yuv10.so, include/vtx_yuv10.h) once, for all
    of its clips; the records are then 24 int32 each, and the 8-bit clips' bytes are those of the other route."""
    return _clips_views('clips_views_yuv', True, clips, frames, left, width, xtab, ytab, out, widths, table)


def yuv420_to_rgb_u8(clip, out=None):
    """The plain conversion of one ``YUVClip`` -> uint8 [Ts,Hs,Ws,3] (include/vtx_yuv.h, of a 10-bit clip include/vtx_yuv10.h:
    nearest chroma siting, the clip's integer matrix), for callers that want the RGB frames.  ``out``: a contiguous uint8
    [Ts,Hs,Ws,3] device tensor to write into."""
    if not isinstance(clip, YUVClip):
        raise TypeError(f'yuv420_to_rgb_u8: a YUVClip is expected, got {type(clip).__name__}')
    need_cuda(*clip.planes)
    Ts, Hs, Ws = clip.shape
    if out is None:
        out = torch.empty(Ts, Hs, Ws, 3, dtype=torch.uint8, device=clip.device)
    else:
        need_cuda(out)
        if out.dtype != torch.uint8 or tuple(out.shape) != (Ts, Hs, Ws, 3) or not out.is_contiguous():
            raise TypeError(f'yuv420_to_rgb_u8: out must be a contiguous uint8 {(Ts, Hs, Ws, 3)} tensor, got {out.dtype} {tuple(out.shape)}')
    if clip.depth == 10:
        rec = upload_i32(clip.record10(), clip.device)
        with _timed('yuv10_to_rgb', nbytes=Ts * clip.source_bytes + out.numel(), key=f'{Ts}x{Hs}x{Ws}'):
            _lib.yuv10_call('vtx_yuv10_to_rgb_u8', ptr(rec), Ts, Hs, Ws, ptr(out), stream())
        return out
    rec = upload_i32(clip.record(), clip.device)
    with _timed('yuv420_to_rgb', nbytes=Ts * (Hs * Ws + 2 * ((Hs + 1) // 2) * ((Ws + 1) // 2)) + out.numel(), key=f'{Ts}x{Hs}x{Ws}'):
        _lib.yuv_call('vtx_yuv420_to_rgb_u8', ptr(rec), Ts, Hs, Ws, ptr(out), stream())
    return out


# ------------------------------------------------- clip-batch mixing, accuracy (csrc/head.hip)
def mixup_batch_(x, lam):
    """In place: x[b] = x[b]*lam + x[B-1-b]*(1-lam) on a contiguous fp32 [B, ...] batch (reference mixup.py:112-113)."""
    need_cuda(x)
    if x.dtype != torch.float32 or not x.is_contiguous():
        raise TypeError('mixup_batch_: contiguous float32 batch required')
    import numpy as np
    B = x.shape[0]
    # ATen multiplies a float32 tensor by a Python scalar after casting the scalar to float32
    call('vtx_mixup_batch', ptr(x), B, x.numel() // B, float(np.float32(lam)), float(np.float32(1. - lam)), stream())
    return x


def cutmix_batch_(x, yl, yh, xl, xh):
    """In place: x[:, :, yl:yh, xl:xh] = x.flip(0)[:, :, yl:yh, xl:xh] on a contiguous fp32 [B, planes, H, W] batch."""
    need_cuda(x)
    if x.dtype != torch.float32 or not x.is_contiguous() or x.ndim != 4:
        raise TypeError('cutmix_batch_: contiguous float32 [B, planes, H, W] batch required')
    B, Pn, H, W = x.shape
    call('vtx_cutmix_batch', ptr(x), B, Pn, H, W, int(yl), int(yh), int(xl), int(xh), stream())
    return x


def cutmix_batch_u8_(clip, yl, yh, xl, xh):
    """In place: clip[:, :, yl:yh, xl:xh] = clip.flip(0)[:, :, yl:yh, xl:xh] on a contiguous uint8 [B,T,H,W,3] batch -- CutMix
    before ToTensor + Normalize, which act per sample (libvtx_mix.so: vtx_cutmix_batch_u8)."""
    need_cuda(clip)
    if clip.dtype != torch.uint8 or not clip.is_contiguous() or clip.ndim != 5 or clip.shape[-1] != 3:
        raise TypeError('cutmix_batch_u8_: contiguous uint8 [B,T,H,W,3] batch required')
    B, T, H, W, _ = clip.shape
    _lib.mix_call('vtx_cutmix_batch_u8', B, T, H, W, ptr(clip), int(yl), int(yh), int(xl), int(xh), stream())
    return clip


def mixup_target(labels, num_classes, lam, smoothing):
    """Label-smoothed one-hot rows mixed with the flipped batch's (reference mixup.py:20-25) -> fp32 [B, num_classes]."""
    import numpy as np
    need_cuda(labels)
    labels = labels.long().contiguous().view(-1)
    B = labels.numel()
    off = smoothing / num_classes
    on = 1. - smoothing + off
    out = torch.empty(B, num_classes, dtype=torch.float32, device=labels.device)
    call('vtx_mixup_target', ptr(labels), B, int(num_classes), float(np.float32(on)), float(np.float32(off)),
         float(np.float32(lam)), float(np.float32(1. - lam)), ptr(out), stream())
    return out


def topk_correct(scores, labels, k, counter):
    """counter (int32 device scalar) += rows of fp32 ``scores`` [B,C] whose label ranks among the k largest."""
    need_cuda(scores, labels, counter)
    scores = scores.float().contiguous()
    labels = labels.long().contiguous()
    B, Cn = scores.shape
    call('vtx_topk_correct', ptr(scores), ptr(labels), B, Cn, int(k), ptr(counter), stream())


def gelu_grad_mul(dy, h, out):
    """out = dy * gelu'(h) elementwise (same shapes / dtype, numel % 8 == 0)."""
    need_cuda(dy, h, out)
    call('vtx_gelu_grad_mul', dt(dy), dy.numel(), ptr(dy), ptr(h), ptr(out), stream())
