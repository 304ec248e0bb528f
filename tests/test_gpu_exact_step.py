"""Exact parity of the kernels either side of the backbone in a training step: csrc/head.hip, the MaskFeat half of csrc/hog.hip
and csrc/optim.hip (helpers and derivations: tests/exact_step.py; premises: tests/test_exact_step_premise.py).

Every output lives in a sentinel-filled buffer with guard elements either side; the in-place kernels work on a tensor inside a
larger flat buffer.  Paths reached (properties of the launch code):
  mixup / cutmix      [2, 3, 1184, 1184]: 1 051 392 float4 per clip (4 205 568 box elements) against a grid of 4096 x 256
                      threads -- the grid-stride loop makes a second trip with a ragged end; B = 2 and 8 at 4 and 8 floats per clip
  mixup_target        1026 x 1024 > 4096 x 256 elements; C = 1; labels equal to the flipped batch's
  cross-entropy       C = 1, 2, 7 (idle lanes), 63, 64, 65 (the second trip of the lane loop starts), 174, 400, 1000; B = 5, 7, 13,
                      257, 1030: ragged last workgroup of 4 rows; 257 and 1030 rows: mean_rows_kernel loops over rows
  top-k               the same shapes; k = 1, 5, C, C + 3
  blend forward       rows C / 8 = 2 408 448 > 8192 x 256 (bf16, every finite bf16 pattern as input); backward 275 968 rows > 1024 x 256
  masked MSE          9408 cells > 2048 workgroups x 4 waves; Cf = 108 and 128: the second trip of the lane loop; ldp, lddp > ts Cf;
                      backward 2 370 816 elements > 8192 x 256
  optimizer           301 tensors (> 256: mt_norms_kernel loops), one of them empty; full chunks on the vector path and, through
                      each of the four pointers alone, on the scalar path; first_step 0 and 1; clip coefficients 2^-6, 2^-5, none
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import exact as X
import exact_step as S
from helpers import report

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
f32 = lambda v: float(np.float32(v))         # noqa: E731


def dev(t, dtype=None):
    return (t if dtype is None else t.to(dtype)).to(DEV).contiguous()


def in_flat(x, dtype=None):
    """x inside a sentinel-guarded flat device buffer -> (view of the shape of x, guards)."""
    x = x if dtype is None else x.to(dtype)
    _, body, guards = S.flat_guarded(x.numel(), DEV, x.dtype)
    body.copy_(x.reshape(-1))
    assert body.data_ptr() % 16 == 0
    return body.view(x.shape), guards


def out_flat(shape, dtype=F32):
    _, body, guards = S.flat_guarded(int(np.prod(shape)), DEV, dtype)
    return body.view(shape), guards


# ============================================================================================ Mixup / CutMix
BIG = (2, 3, 1184, 1184)


@functools.lru_cache(maxsize=1)
def _big_clip():
    return torch.randn(BIG, generator=X.gen(0))


def _mixup_ref(x, lam):
    ref = x.clone()
    flipped = ref.flip(0).mul_(1. - lam)                     # the reference's ATen calls
    return ref.mul_(lam).add_(flipped)


def _cutmix_ref(x, yl, yh, xl, xh):
    ref = x.clone()
    ref[:, :, yl:yh, xl:xh] = ref.flip(0)[:, :, yl:yh, xl:xh]
    return ref


def test_mixup_and_cutmix_beyond_the_grid_cap():
    from vtx import ops
    x = _big_clip()
    assert x[0].numel() // 4 * (BIG[0] // 2) > 4096 * 256
    for lam in (0.3141592, 0.9, 0.5):
        view, guards = in_flat(x)
        ops.mixup_batch_(view, lam)
        X.check_exact(f'mixup {BIG} lam={lam}', view, _mixup_ref(x, lam), guards)
    H, W = BIG[2:]
    for box in ((0, H, 0, W), (0, H, 500, 501), (700, H, 600, W)):
        view, guards = in_flat(x)
        ops.cutmix_batch_(view, *box)
        X.check_exact(f'cutmix {BIG} box={box}', view, _cutmix_ref(x, *box), guards)


@pytest.mark.parametrize('B', [2, 8])
@pytest.mark.parametrize('per_clip', [4, 8])
def test_mixup_and_cutmix_small_batches(B, per_clip):
    from vtx import ops
    x = torch.randn(B, per_clip // 4, 2, 2, generator=X.gen(B + per_clip))
    for lam in (0.3141592, 0.9, 0.5):
        view, guards = in_flat(x)
        ops.mixup_batch_(view, lam)
        X.check_exact(f'mixup B={B} per_clip={per_clip} lam={lam}', view, _mixup_ref(x, lam), guards)
    for box in ((0, 2, 0, 2), (1, 2, 0, 1), (0, 1, 1, 2)):
        view, guards = in_flat(x)
        ops.cutmix_batch_(view, *box)
        X.check_exact(f'cutmix B={B} per_clip={per_clip} box={box}', view, _cutmix_ref(x, *box), guards)


def test_odd_batch_is_refused_not_mixed():
    """vtx_mixup_batch / vtx_cutmix_batch answer an odd batch with VTX_EINVAL (-1) and touch nothing; mixup.Mixup refuses it the
    way the reference's class does (an AssertionError naming the even batch)."""
    import mixup
    import vtx
    from vtx import ops
    x = torch.randn(3, 2, 2, 2, generator=X.gen(1))
    view, guards = in_flat(x)
    with pytest.raises(vtx._lib.VtxError, match=r'code -1'):
        ops.mixup_batch_(view, 0.3)
    with pytest.raises(vtx._lib.VtxError, match=r'code -1'):
        ops.cutmix_batch_(view, 0, 2, 0, 2)
    with pytest.raises(AssertionError, match='Batch size should be even'):
        mixup.Mixup(num_classes=5)(view, torch.tensor([0, 1, 2], device=DEV))
    X.check_exact('odd batch untouched', view, x, guards)


def _target_ref(labels, Cn, lam, smoothing):
    off = smoothing / Cn
    on = 1. - smoothing + off
    oh = lambda t: torch.full((t.numel(), Cn), off).scatter_(1, t.view(-1, 1), on)   # noqa: E731
    return oh(labels) * lam + oh(labels.flip(0)) * (1. - lam), on, off


@pytest.mark.parametrize('B,Cn', [(1026, 1024), (6, 1), (8, 10)])
def test_mixup_target_exact(B, Cn):
    import vtx
    from vtx import ops
    labels = torch.randint(0, Cn, (B,), generator=X.gen(B))
    labels[B - 1] = labels[0]                                # rows whose label equals the flipped batch's
    labels[B - 2] = labels[1]
    assert B * Cn > 4096 * 256 or B < 10
    for lam, smoothing in ((0.37, 0.1), (1.0, 0.0), (0.8123, 0.2)):
        ref, on, off = _target_ref(labels, Cn, lam, smoothing)
        out, guards = out_flat((B, Cn))
        vtx._lib.call('vtx_mixup_target', ops.ptr(dev(labels)), B, Cn, f32(on), f32(off), f32(lam), f32(1. - lam), ops.ptr(out), ops.stream())
        X.check_exact(f'mixup_target {B}x{Cn} lam={lam}', out, ref, guards)
        assert torch.equal(ops.mixup_target(dev(labels), Cn, lam, smoothing).cpu(), ref)


# =========================================================================================== cross-entropy
def run_xent(x, target, gloss=S.GLOSS):
    """Forward and backward through the C API on guarded buffers -> (outputs on the CPU, guards)."""
    import vtx
    from vtx import ops
    B, Cn = x.shape
    soft = target.is_floating_point()
    xd, td = dev(x), dev(target)
    (rows, g1), (lse, g2), (mean, g3), (dx, g4) = out_flat((B,)), out_flat((B,)), out_flat((2,)), out_flat((B, Cn))
    vtx._lib.call('vtx_softmax_xent_fwd', ops.ptr(xd), ops.ptr(td) if soft else None, None if soft else ops.ptr(td), B, Cn,
                  ops.ptr(rows), ops.ptr(lse), ops.ptr(mean), ops.stream())
    gl = torch.tensor([gloss], dtype=F32, device=DEV)
    vtx._lib.call('vtx_softmax_xent_bwd', ops.ptr(xd), ops.ptr(td) if soft else None, None if soft else ops.ptr(td), ops.ptr(lse),
                  B, Cn, 1.0, ops.ptr(gl), mean.data_ptr() + 4, ops.ptr(dx), ops.stream())
    torch.cuda.synchronize()
    guards = {f'{n} {k}': v for n, g in (('rows', g1), ('lse', g2), ('mean', g3), ('dx', g4)) for k, v in g.items()}
    return dict(rows=rows.cpu(), lse=lse.cpu(), mean=mean[0].cpu(), count=mean[1].cpu(), dx=dx.cpu()), guards


@pytest.mark.parametrize('B,Cn', S.XENT_SHAPES)
def test_xent_structure_exact(B, Cn):
    """One finite term per row: lse, every row loss, the mean (one rounded division) and dx are unique; so are the ignored rows,
    the all-ignored batch (mean NaN, dx 0) and the count."""
    from vtx import functions as F_
    for mode in S.XENT_STRUCTURE_MODES:
        c = S.xent_structure_case(B, Cn, mode, seed=B + Cn)
        got, guards = run_xent(c['x'], c['target'])
        X.check_exact(c['name'] + ' rows', got['rows'], c['rows'], guards)
        X.check_exact(c['name'] + ' lse', got['lse'], c['lse'])
        X.check_exact(c['name'] + ' mean', got['mean'], c['mean'])
        X.check_exact(c['name'] + ' count', got['count'], torch.tensor(float(c['count'])))
        X.check_exact(c['name'] + ' dx', got['dx'], c['dx'])
        xg = dev(c['x']).requires_grad_(True)                 # and through the autograd Function
        loss = F_.SoftmaxXentFn.apply(xg, dev(c['target']))
        (loss * S.GLOSS).backward()
        X.check_exact(c['name'] + ' Fn loss', loss.detach(), c['mean'])
        X.check_exact(c['name'] + ' Fn dx', xg.grad, c['dx'])


@pytest.mark.parametrize('B,Cn', S.XENT_SHAPES)
def test_xent_accuracy_bound(B, Cn):
    """Dyadic random logits at spreads 3 and 30 and offsets 0, -64, 64, 4096: row losses, mean and dx within the derived
    per-element bound at K_GPU = 2 K_REF.  Before the kernels subtracted the row maximum first the offset cases missed it
    (MI355X, labels 257 x 400 s = 3: offset 64 rows k = 12.7, dx k = 49.8; offset 4096 rows k = 859, dx k = 3228); now every offset
    gives the same figures (rows k = 1.16, dx k = 0.96)."""
    failed = []
    for s, off, tgt in S.XENT_ACCURACY:
        c = S.xent_accuracy_case(B, Cn, s, off, tgt, seed=B * Cn + s)
        got, guards = run_xent(c['x'], c['target'])
        assert not any(X.sentinel_touched(g) for g in guards.values()), c['name']
        try:
            S.xent_check(c['name'], got, S.xent_f64(c['x'], c['target']), S.K_GPU)
        except AssertionError as e:
            failed.append(str(e))
    assert not failed, '\n'.join(failed)


# =================================================================================================== top-k
def _counter(start):
    _, body, guards = S.flat_guarded(4, DEV)
    cnt = body.view(torch.int32)[:1]
    cnt.fill_(start)
    guards['rest'] = body[1:]
    return cnt, guards


@pytest.mark.parametrize('B,Cn', S.XENT_SHAPES)
def test_topk_tie_rule_exact(B, Cn):
    """Equality with the stated rule on tie-heavy rows with +-inf and ignored labels, with torch.topk on tie-free rows; the
    counter accumulates over two calls from a non-zero start."""
    from vtx import ops
    for k in S.topk_ks(Cn):
        s, lab = S.topk_tie_case(B, Cn, k, seed=B + Cn + k)
        want = S.topk_ref(s, lab, k)
        cnt, guards = _counter(7)
        sd, ld = dev(s), dev(lab)
        ops.topk_correct(sd, ld, k, cnt)
        ops.topk_correct(sd, ld, k, cnt)
        got = int(cnt.item())
        bad = got != 7 + 2 * want or any(X.sentinel_touched(g) for g in guards.values())
        report(f'{"FAIL" if bad else "ok  "} exact topk ties {B}x{Cn} k={k}: counter {got} (7 + 2 x {want})')
        assert not bad, (k, got, want)
        s, lab = S.topk_free_case(B, Cn, seed=B + Cn)
        want = int((s.topk(min(k, Cn), dim=-1).indices == lab[:, None]).any(-1).sum())
        assert want == S.topk_ref(s, lab, k)
        cnt, _ = _counter(0)
        ops.topk_correct(dev(s), dev(lab), k, cnt)
        assert int(cnt.item()) == want, ('tie-free', k, int(cnt.item()), want)


def test_topk_nan_scores_reported():
    from vtx import ops
    s, lab = S.topk_tie_case(257, 400, 5, seed=3)
    s[::5, 7] = float('nan')
    s[3, :] = float('nan')
    cnt, _ = _counter(0)
    ops.topk_correct(dev(s), dev(lab), 5, cnt)
    report(f'ok   topk with NaN scores (not asserted): counter {int(cnt.item())}, the comparison rule gives {S.topk_ref(s, lab, 5)}')


# ================================================================================================ MaskFeat
def _blend(kind, dtype, B, Tq, Hq, Cn, g, a, mask, tok_or_dtok, out):
    import vtx
    from vtx import ops
    vtx._lib.call(f'vtx_maskfeat_blend_{kind}', ops.dt(out), B, Tq, Hq, Hq, Cn, g, ops.ptr(a), ops.ptr(mask),
                  *((ops.ptr(tok_or_dtok), ops.ptr(out)) if kind == 'fwd' else (ops.ptr(out), ops.ptr(tok_or_dtok))), ops.stream())
    torch.cuda.synchronize()


BLEND_SMALL = [(2, 2, 3, r, Cn) for Cn in (8, 96) for r in (1, 2, 4)]


@pytest.mark.parametrize('dtype', [BF16, F32])
def test_maskfeat_blend_forward_exact(dtype):
    shapes = [(s, k) for s in BLEND_SMALL for k in ('zeros', 'ones', 'random')]
    if dtype == BF16:
        shapes.append(((6, 8, 14, 16, 8), 'random'))         # 224 x 224 tokens: 2 408 448 groups of 8 > 8192 x 256
    for (B, Tq, g, r, Cn), kind in shapes:
        Hq = g * r
        rows = B * Tq * Hq * Hq
        assert rows < 10 ** 5 or rows * Cn // 8 > 8192 * 256
        x = S.mf_blend_x(rows, Cn, dtype)
        mask = S.mf_mask(B, Tq, g, kind, seed=Cn + r)
        tok = S.mf_token(Cn, seed=Cn)
        tok_out = X.expect_bf16('mask token', tok, 'round') if dtype == BF16 else tok.float()
        want = torch.where(S.mf_expand(mask, r)[:, None], tok_out[None, :], x)
        out, guards = out_flat((rows, Cn), dtype)
        _blend('fwd', dtype, B, Tq, Hq, Cn, g, dev(x), dev(mask), dev(tok.float()), out)
        X.check_exact(f'maskfeat blend fwd {dtype} B={B} Tq={Tq} {Hq}x{Hq} C={Cn} mask={kind}', out, want, guards)


@pytest.mark.parametrize('dtype', [BF16, F32])
def test_maskfeat_blend_backward_exact(dtype):
    """dy small integers: every partial sum of dtoken is an integer below 2^24, so the atomics give one answer in any order;
    dtoken is sentinel-filled on entry (the entry point clears it); dx is dy or 0."""
    for B, Tq, g, r, Cn in BLEND_SMALL + [(11, 8, 14, 4, 8)]:    # 56 x 56 tokens: 275 968 rows > 1024 x 256
        Hq = g * r
        rows = B * Tq * Hq * Hq
        assert rows < 10 ** 4 or rows > 1024 * 256
        dy = X.ints((rows, Cn), -4, 4, 1.0, rows + Cn)
        mask = S.mf_mask(B, Tq, g, 'random', seed=Cn + r)
        mrow = S.mf_expand(mask, r)
        dtok = (dy.double() * mrow[:, None]).sum(0)
        assert float((dy.abs() * mrow[:, None]).sum(0).max()) < X.EXACT_LIMIT
        dx, guards = out_flat((rows, Cn), dtype)
        dtoken, g2 = out_flat((Cn,))
        _blend('bwd', dtype, B, Tq, Hq, Cn, g, dev(dy, dtype), dev(mask), dtoken, dx)
        name = f'maskfeat blend bwd {dtype} B={B} Tq={Tq} {Hq}x{Hq} C={Cn}'
        X.check_exact(name + ' dx', dx, torch.where(mrow[:, None], torch.zeros_like(dy), dy).to(dtype), guards)
        X.check_exact(name + ' dtoken', dtoken, dtok.float(), g2)


def _acc():
    _, body, guards = S.flat_guarded(4, DEV)
    return body.view(F64), guards


MF_LOSS = [(1, 2, 2, 14, Cf, n) for Cf in (64, 128, 24, 108) for n in (0, 1, 255, 256, 300)] + \
          [(3, 8, 2, 14, 128, 5000), (3, 8, 2, 14, 108, 5000)]           # 9408 cells > 8192
MF_LOSS_BWD_BIG = (7, 8, 2, 14, 108, 9000)                               # 2 370 816 elements > 8192 x 256


@pytest.mark.parametrize('dtype', [BF16, F32])
def test_maskfeat_loss_exact(dtype):
    """Dyadic pred / target: with Cf a power of two both accumulators are unique (equality), otherwise 1e-12 relative; the
    gradient is the replay T(float32(coef (pred - target))) by equality for every count, with ldp, lddp > ts Cf."""
    import vtx
    from vtx import ops
    gloss = 0.75
    for B, Tq, ts, g, Cf, n in MF_LOSS + [MF_LOSS_BWD_BIG]:
        c = S.mf_loss_case(B, Tq, ts, g, Cf, n, dtype, pad=8, seed=Cf + n)
        name = f'maskfeat loss {dtype} B={B} Tq={Tq} ts={ts} g={g} Cf={Cf} masked={n}'
        pd, tg, cm = dev(c['pred'], dtype), dev(c['target']), dev(c['cmask'])
        assert pd.shape == (c['rows'], c['ldp']) and tg.numel() == c['cells'] * Cf and cm.numel() == c['cells']
        acc, guards = _acc()
        vtx._lib.call('vtx_maskfeat_loss_fwd', ops.dt(pd), B, Tq, ts, g, Cf, ops.ptr(pd), c['ldp'], ops.ptr(tg), ops.ptr(cm), ops.ptr(acc),
                      ops.stream())
        torch.cuda.synchronize()
        got = acc.cpu()
        want = torch.stack([c['loss'], torch.tensor(float(n), dtype=F64)])
        if c['exact']:
            X.check_exact(name + ' acc', got, want, guards)
        else:
            rel = abs(float(got[0]) - float(want[0])) / max(float(want[0]), 1e-300) if n else abs(float(got[0]))
            bad = rel >= 1e-12 or float(got[1]) != n or any(X.sentinel_touched(v) for v in guards.values())
            report(f'{"FAIL" if bad else "ok  "} {name} acc: rel={rel:.2e} (tol 1e-12), count {float(got[1]):g}')
            assert not bad, (name, got, want)
        lddp = ts * Cf + 4
        dp, g2 = out_flat((c['rows'], lddp), dtype)
        vtx._lib.call('vtx_maskfeat_loss_bwd', ops.dt(pd), B, Tq, ts, g, Cf, ops.ptr(pd), c['ldp'], ops.ptr(tg), ops.ptr(cm), ops.ptr(acc),
                      gloss, ops.ptr(dp), lddp, ops.stream())
        torch.cuda.synchronize()
        g2['ld padding'] = dp[:, ts * Cf:]
        X.check_exact(name + ' dpred', dp[:, :ts * Cf], S.mf_loss_bwd_expected(c, gloss, dtype), g2)


# =============================================================================================== optimizer
@functools.lru_cache(maxsize=1)
def _lay():
    return S.MtLayout()


class Table:
    """The layout's tensors in flat device buffers and a hand-built vtx_mt_tensor table over them."""

    def __init__(self, lay, groups, packed):
        import vtx
        self.lay, self.lib = lay, vtx._lib
        self.bufs = [None if t is None else dev(X.sentinel_fill(torch.empty(lay.total[j])) if isinstance(t, str) else lay.flat(j, t))
                     for j, t in enumerate(packed)]
        assert all(b is None or b.data_ptr() % 16 == 0 for b in self.bufs)
        self.tab = (vtx._lib.MtTensor * lay.n)()
        starts = [0]
        for t in range(lay.n):
            for j, f in enumerate(('p', 'g', 's1', 's2')):
                setattr(self.tab[t], f, None if self.bufs[j] is None else self.bufs[j].data_ptr() + 4 * int(lay.pos[t, j]))
            self.tab[t].n = lay.sizes[t]
            starts.append(starts[-1] + lay.chunks[t])
            assert self.lib.load().vtx_mt_chunks(lay.sizes[t]) == lay.chunks[t]
        self.n_chunks = starts[-1]
        self.starts = torch.tensor(starts, dtype=torch.int32).to(DEV)
        self.tab_dev = torch.empty(C.sizeof(self.tab), dtype=torch.uint8, device=DEV)
        self.partial, self.g_partial = out_flat((self.n_chunks,))
        self.norms, self.g_norms = out_flat((lay.n + 1,))
        self.set_hyper(groups)

    def set_hyper(self, groups):
        for t in range(self.lay.n):
            self.tab[t].lr, self.tab[t].wd = groups[self.lay.group[t]]
        self.tab_dev.copy_(torch.frombuffer(bytearray(bytes(self.tab)), dtype=torch.uint8))

    def upload(self, j, packed):
        self.bufs[j].copy_(self.lay.flat(j, packed))

    def call(self, name, *args):
        from vtx import ops
        head = (self.tab_dev.data_ptr(), self.starts.data_ptr(), self.lay.n, self.n_chunks)
        if name == 'vtx_mt_grad_norms':
            self.lib.call(name, *head, ops.ptr(self.partial), ops.ptr(self.norms), ops.stream())
        else:
            self.lib.call(name, *head, ops.ptr(self.norms), *args, ops.stream())
        torch.cuda.synchronize()

    def check(self, name, j, packed):
        """Buffer j holds the packed expected values and the sentinel everywhere else, bit for bit."""
        got = self.bufs[j].cpu()
        outside = torch.ones(self.lay.total[j], dtype=torch.bool)
        outside[self.lay.index[j]] = False
        X.check_exact(name, got, self.lay.flat(j, packed), {'between the tensors': got[outside]})

    def packed(self, j):
        return self.lay.packed(j, self.bufs[j]).double()

    def guards_touched(self, j):
        outside = torch.ones(self.lay.total[j], dtype=torch.bool)
        outside[self.lay.index[j]] = False
        return X.sentinel_touched(self.bufs[j].cpu()[outside])


@pytest.mark.parametrize('kind', ['ints', 'clip'])
def test_grad_norms_exact(kind):
    """Sums of squares exact in any order: norms[t] = float32(sqrt(sum)) for 301 tensors (one empty, a third misaligned), the last
    entry the same over the total; norms of exactly 64 and 32 among them."""
    lay = _lay()
    g = S.mt_grads(lay, kind)
    want, _ = S.mt_norms_expected(lay, g)
    tb = Table(lay, S.MT_GROUPS, (S.mt_params(lay), g, None, None))
    tb.call('vtx_mt_grad_norms')
    X.check_exact(f'mt norms [{kind}]', tb.norms, want, {**tb.g_norms, **{'partial ' + k: v for k, v in tb.g_partial.items()}})
    tb.check(f'mt norms [{kind}] gradients untouched', 1, g)


@pytest.mark.parametrize('clip', [0.0, 1.0])
@pytest.mark.parametrize('nesterov', [1, 0])
@pytest.mark.parametrize('first', [0, 1])
def test_sgd_exact(clip, nesterov, first):
    """Two steps in exact arithmetic (lr 2^-4 / 2^-3, wd 0 / 0.5, momentum 0.5); first_step = 1 starts from a momentum buffer full
    of NaN, which it must not read; clip = 1 with norms 64, 32, <= 0.5 and 0."""
    lay = _lay()
    tb = Table(lay, S.MT_GROUPS, (S.mt_params(lay), S.mt_params(lay), 'sentinel' if first else torch.zeros(lay.numel), None))
    for step, (p, m, g, norms) in enumerate(S.sgd_exact_expected(lay, clip, nesterov, first)):
        tb.upload(1, g)
        name = f'sgd exact clip={clip} nesterov={nesterov} first_step={first} step {step}'
        if clip:
            tb.call('vtx_mt_grad_norms')
            X.check_exact(name + ' norms', tb.norms, norms, tb.g_norms)
        tb.call('vtx_mt_sgd_step', clip, 0.5, nesterov, int(bool(first and step == 0)))
        tb.check(name + ' p', 0, p)
        tb.check(name + ' momentum', 2, m)


@pytest.mark.parametrize('wd_on', [False, True])
@pytest.mark.parametrize('preload', [False, True])
def test_adamw_exact(wd_on, preload):
    """Step 1 with betas (0.5, 0.75), eps 2^-10, lr 2^-4: every product exact, so m and v are exact and p is the float32 replay
    (one correctly rounded sqrt, division, + eps and subtraction per element).  From zero state (sqrt(v) = |g| / 2 exact) p equals
    the replay everywhere.  With preloaded m, v, where sqrt(v) is inexact, the MI355X build differs from the replay by one ulp
    on 0.5 % of the elements (4670 / 4681 of 905 144): those elements are counted, reported and held to the
    per-element bound of the general steps; every other element is held by equality."""
    lay = _lay()
    c = S.adamw_exact_case(lay, wd_on, preload)
    tb = Table(lay, c['groups'], (c['p0'], c['g'], c['m0'], c['v0']))
    tb.call('vtx_mt_adamw_step', 0.0, S.ADAMW_EXACT['b1'], S.ADAMW_EXACT['b2'], S.ADAMW_EXACT['eps'], 1)
    name = f'adamw exact wd={"on" if wd_on else "off"} preload={preload}'
    tb.check(name + ' m', 2, c['m'])
    tb.check(name + ' v', 3, c['v'])
    if not preload:
        tb.check(name + ' p', 0, c['p'])
        return
    got = dict(p=tb.packed(0), m=tb.packed(2), v=tb.packed(3))
    off = X.mismatch(got['p'].float(), c['p'].float())
    n_off = int(off.sum())
    assert tb.guards_touched(0) == 0
    if n_off:
        lr, wd = lay.hyper(c['groups'])
        ref = S.general_step64('adamw', c['p0'], c['g'], c['m0'], c['v0'], torch.ones_like(c['p0']), lr, wd,
                               S.adamw_hyper(step=1, **S.ADAMW_EXACT))
        big = torch.maximum(got['p'].abs(), c['p'].abs())[off]
        ulps = float(((got['p'] - c['p'])[off].abs() / 2.0 ** (torch.floor(torch.log2(big)) - 23)).max())
        report(f'ok   {name} p: {n_off} of {off.numel()} elements off the float32 replay, by at most {ulps:.2f} ulp of p '
               f'(one ulp of the quotient, seen through the rounding of the final subtraction)')
        grp = torch.tensor(lay.group)[lay.tid]
        for gi in (0, 1):
            S.opt_check(f'{name} p, elements off the replay, group {gi}', 'adamw', got, ref, 2 * S.K_OPT['adamw'][gi], sel=off & (grp == gi))
        assert n_off <= 0.01 * off.numel(), f'{n_off} elements off the replay: more than a rare one-ulp quotient'
    else:
        report(f'ok   {name} p: equal to the float32 replay everywhere')


@pytest.mark.parametrize('kind', ['sgd', 'adamw'])
def test_general_steps_bound(kind):
    """Four general steps (the reference's hyper-parameters, a scheduler rewrite before the third, clip 0.5): after each, every
    element of p, m, v within the per-element bound of the float64 step from the state the kernel started from; the norms
    within 17 u (per tensor: <= 31 roundings of the sum, halved by the sqrt, plus its own) and 23 u (norm of norms)."""
    lay = _lay()
    groups = [list(gp) for gp in S.MT_GROUPS_GENERAL[kind]]
    clip = 0.5
    z = torch.zeros(lay.numel)
    tb = Table(lay, groups, (S.general_data(lay, kind, -1), z, z, z if kind == 'adamw' else None))
    grp = torch.tensor(lay.group)[lay.tid]
    for step in range(4):
        if step == 2:
            groups[1][1] = 0.02
            groups[0][0] *= 0.5
            tb.set_hyper(groups)
        g = S.general_data(lay, kind, step)
        tb.upload(1, g)
        p0, m0 = tb.packed(0), tb.packed(2)
        v0 = tb.packed(3) if kind == 'adamw' else None
        tb.call('vtx_mt_grad_norms')
        norms = tb.norms.cpu().double()
        sq = torch.zeros(lay.n, dtype=F64).index_add_(0, lay.tid, g * g)
        n64 = torch.cat([sq.sqrt(), sq.sum().sqrt().reshape(1)])
        rel = ((norms - n64).abs() / n64.clamp_min(1e-300))
        report(f'ok   {kind} general step {step} norms: worst {float(rel[:-1].max()) / S.U24:.2f} u, total {float(rel[-1]) / S.U24:.2f} u')
        assert float(rel[:-1].max()) <= 17 * S.U24 and float(rel[-1]) <= 23 * S.U24
        c = f32(clip) / (norms[:-1] + float(np.float32(1e-6)))
        coef = lay.per_element(torch.where(c < 1, c, torch.ones_like(c)))
        lr, wd = lay.hyper(groups)
        if kind == 'sgd':
            h = dict(mom=f32(0.9))
            tb.call('vtx_mt_sgd_step', clip, 0.9, 1, 0)
        else:
            h = S.adamw_hyper(0.9, 0.999, 1e-8, step + 1)
            tb.call('vtx_mt_adamw_step', clip, 0.9, 0.999, 1e-8, step + 1)
        ref = S.general_step64(kind, p0, g, m0, v0, coef, lr, wd, h)
        got = dict(p=tb.packed(0), m=tb.packed(2))
        if kind == 'adamw':
            got['v'] = tb.packed(3)
        failed = []
        for gi in (0, 1):
            try:
                S.opt_check(f'{kind} general step {step} group {gi}', kind, got, ref, 2 * S.K_OPT[kind][gi], sel=grp == gi)
            except AssertionError as e:
                failed.append(str(e))
        assert not failed, '\n'.join(failed)
    for j in (0, 2, 3) if kind == 'adamw' else (0, 2):
        assert tb.guards_touched(j) == 0, f'buffer {j}: guard elements between the tensors overwritten'


def _class_params(lay, tb):
    """Parameters that are views of the table's flat buffers (misaligned ones included), gradients likewise."""
    ps = []
    for t in range(lay.n):
        a, b = int(lay.pos[t, 0]), int(lay.pos[t, 1])
        p = torch.nn.Parameter(tb.bufs[0][a:a + lay.sizes[t]])
        p.grad = tb.bufs[1][b:b + lay.sizes[t]]
        ps.append(p)
    return ps


def test_fused_sgd_class_matches_the_raw_table():
    """FusedSGD over 301 parameters in two groups with clip_grad = 1: the expected values of the raw-table run, by equality."""
    from vtx import optim
    lay = _lay()
    tb = Table(lay, S.MT_GROUPS, (S.mt_params(lay), S.mt_params(lay), None, None))
    ps = _class_params(lay, tb)
    o = optim.FusedSGD([{'params': ps[0::2], 'lr': S.MT_GROUPS[0][0], 'weight_decay': S.MT_GROUPS[0][1]},
                        {'params': ps[1::2], 'lr': S.MT_GROUPS[1][0], 'weight_decay': S.MT_GROUPS[1][1]}],
                       lr=1.0, momentum=0.5, nesterov=True, clip_grad=1.0)
    for step, (p, m, g, norms) in enumerate(S.sgd_exact_expected(lay, 1.0, 1, 0)):
        tb.upload(1, g)
        o.step()
        torch.cuda.synchronize()
        tb.check(f'FusedSGD step {step} p', 0, p)
        got_m = torch.cat([o.state[q]['momentum_buffer'].reshape(-1) for q in ps]).cpu()
        X.check_exact(f'FusedSGD step {step} momentum', got_m, m.float())
        X.check_exact(f'FusedSGD step {step} norm of norms', o.last_grad_norm.cpu(), norms[-1])


def test_fused_adamw_class_partitions_match_the_raw_table():
    """FusedAdamW over 301 parameters; a fifth of them skipped in the first step, so the second step runs two partitions: those
    taking their first update (equality with the raw-table expectation) and those taking their second (the general bound)."""
    from vtx import optim
    lay = _lay()
    c = S.adamw_exact_case(lay, True, False)
    tb = Table(lay, c['groups'], (c['p0'], c['g'], None, None))
    ps = _class_params(lay, tb)
    o = optim.FusedAdamW([{'params': ps[0::2], 'weight_decay': c['groups'][0][1]}, {'params': ps[1::2], 'weight_decay': c['groups'][1][1]}],
                         lr=c['groups'][0][0], betas=(S.ADAMW_EXACT['b1'], S.ADAMW_EXACT['b2']), eps=S.ADAMW_EXACT['eps'])
    late = torch.tensor([t % 5 == 0 for t in range(lay.n)])[lay.tid]
    o.set_skipped(ps[0::5])
    o.step()
    torch.cuda.synchronize()
    tb.check('FusedAdamW step 1 (a fifth skipped) p', 0, torch.where(late, c['p0'], c['p']))
    o.set_skipped([])
    assert len(o._partition(o._entries())) == 2
    p1 = tb.packed(0)
    m1 = torch.cat([o.state[q]['exp_avg'].reshape(-1) if 'exp_avg' in o.state[q] else torch.zeros(q.numel(), device=DEV) for q in ps]).cpu().double()
    v1 = torch.cat([o.state[q]['exp_avg_sq'].reshape(-1) if 'exp_avg' in o.state[q] else torch.zeros(q.numel(), device=DEV) for q in ps]).cpu().double()
    o.step()
    torch.cuda.synchronize()
    got = dict(p=tb.packed(0), m=torch.cat([o.state[q]['exp_avg'].reshape(-1) for q in ps]).cpu().double(),
               v=torch.cat([o.state[q]['exp_avg_sq'].reshape(-1) for q in ps]).cpu().double())
    for key in ('p', 'm', 'v'):
        X.check_exact(f'FusedAdamW first update of the late partition {key}', got[key][late].float(), c[key][late].float())
    steps = {int(o.state[q]['step']) for q in ps[0::5]}, {int(o.state[q]['step']) for q in ps if q.numel() and not any(q is s for s in ps[0::5])}
    assert steps == ({1}, {2}), steps
    lr, wd = lay.hyper(c['groups'])
    ref = S.general_step64('adamw', p1, c['g'], m1, v1, torch.ones_like(p1), lr, wd, S.adamw_hyper(step=2, **S.ADAMW_EXACT))
    grp = torch.tensor(lay.group)[lay.tid]
    for gi in (0, 1):
        S.opt_check(f'FusedAdamW second update group {gi}', 'adamw', got, ref, 2 * S.K_OPT['adamw'][gi], sel=(grp == gi) & ~late)
