"""CPU checks of the exact training-step test machinery (tests/exact_step.py): the premise of every case that
test_gpu_exact_step.py runs, the measured k of the float32 transcriptions, and that the new checks reject kernel faults that
the tolerance tests of test_gpu_head.py / test_gpu_optim.py / test_maskfeat_kernels let through on the shapes they use
(emulated on the CPU in the arithmetic of the kernels)."""
import functools
import math

import pytest
import torch

import exact as X
import exact_step as S
from helpers import relerr, report

F32, F64 = torch.float32, torch.float64
OLD_XENT_SHAPES = ((64, 400), (5, 174), (3, 7))          # test_gpu_head.py: randn * 3, bars 1e-6 (loss) and 1e-5 (dlogits)
OLD_OPT_SHAPES = [(768, 768), (3,), (4097,), (2304, 768), (1, 1, 768), (5, 7, 11), (8192,), (12288 + 4,)]   # test_gpu_optim.py


# ------------------------------------------------------------------------------------------ cross-entropy
def test_xent_structure_case_premises():
    """The builders assert exactness; here: the arg-max reaches the last column, lane 63's tail element and column 64, counts
    are powers of two in some cases and not in others, ignored labels of all three kinds occur."""
    pow2, ignored, at = set(), set(), set()
    for B, C in S.XENT_SHAPES:
        for mode in S.XENT_STRUCTURE_MODES:
            c = S.xent_structure_case(B, C, mode, seed=B + C)
            pow2.add(c['pow2_count'])
            r = S.xent_f64(c['x'], c['target'])
            assert torch.equal(r['rows'].float(), c['rows']) and torch.equal(r['lse'].float(), c['lse'])
            if mode == 'all_ignored':
                assert c['count'] == 0 and math.isnan(float(c['mean'])) and not c['dx'].any()
            if mode == 'labels':
                ignored |= set(c['target'][~c['valid']].tolist())
                assert bool((c['rows'][c['valid']] == 0).any()) or B < 2, 'a label at the arg-max'
            if C > 64:
                at |= {('last', True)} if (c['argmax'] == C - 1).any() else set()
                at |= {('col64', True)} if (c['argmax'] == 64).any() else set()
                at |= {('lane63 tail', True)} if (c['argmax'] == 63 + 64 * ((C - 64) // 64)).any() else set()
    assert pow2 == {True, False}
    assert {-100, -1} <= ignored and any(v > 0 for v in ignored)
    assert len(at) == 3


@functools.lru_cache(maxsize=None)
def _k_of_transcriptions():
    """k of d = lse - x and of p over every accuracy case, for both forms: {form: {offset: (k_d, k_p)}}."""
    out = {form: {} for form in ('max_first', 'kernel')}
    for B, C in S.XENT_SHAPES:
        for s, off, tgt in S.XENT_ACCURACY:
            if tgt != 'labels':
                continue                                          # d and p depend on the logits only
            c = S.xent_accuracy_case(B, C, s, off, tgt, seed=B * C + s)
            r = S.xent_f64(c['x'], c['target'])
            for form in out:
                d, p, _ = S.xent_terms32(c['x'], form)
                kd = S.k_needed((d.double() - r['d']).abs(), torch.zeros_like(r['d']), S.U24 * (1 + r['d']))
                big = r['p'] > 2.0 ** -100
                kp = S.k_needed(((p.double() - r['p']).abs())[big], torch.zeros_like(r['p'])[big],
                                (S.U24 * (1 + r['d']) * r['p'])[big])
                old = out[form].get(off, (0.0, 0.0))
                out[form][off] = (max(old[0], kd), max(old[1], kp))
    return out


def test_xent_max_first_transcription_stays_within_k_ref():
    """The one measured number: K_REF bounds the float32 max-first transcription on every accuracy case, whatever the offset;
    the form the kernels had before needs hundreds at offset 4096."""
    k = _k_of_transcriptions()
    for form in k:
        for off, (kd, kp) in sorted(k[form].items()):
            report(f'ok   k of the float32 transcription [{form}] offset {off}: d = lse - x needs {kd:.2f}, softmax needs {kp:.2f}')
    worst = max(max(v) for v in k['max_first'].values())
    report(f'ok   xent K_REF = {S.K_REF}: the max-first transcription needs {worst:.2f} over {len(S.XENT_SHAPES)} shapes x '
           f'{len(S.XENT_ACCURACY)} cases')
    assert S.K_REF / 2 < worst <= S.K_REF, f'K_REF = {S.K_REF} is not the next power of two above {worst:.3f}'
    assert S.K_GPU == 2 * S.K_REF
    assert max(k['kernel'][4096]) > 20 * S.K_GPU


@pytest.mark.parametrize('B,C', S.XENT_SHAPES)
def test_xent_replay_passes_the_derived_bound(B, C):
    """The whole pipeline (row losses, mean, dx) of the max-first float32 replay lies within xent_bounds at K_REF on every
    accuracy case: the roundings counted in the derivation cover the arithmetic."""
    worst = {}
    for s, off, tgt in S.XENT_ACCURACY:
        c = S.xent_accuracy_case(B, C, s, off, tgt, seed=B * C + s)
        need, _ = S.xent_check(c['name'], S.xent_replay32(c['x'], c['target']), S.xent_f64(c['x'], c['target']), S.K_REF, quiet=True)
        worst = {k: max(v, worst.get(k, 0.0)) for k, v in need.items()}
        assert max(need.values()) <= S.K_REF, (c['name'], need)
    report(f'ok   xent float32 replay {B}x{C}: ' + ', '.join(f'{k} k={v:.2f}' for k, v in worst.items()) + f' (K_REF {S.K_REF})')


def _old_xent_inputs(B, C):
    g = torch.Generator().manual_seed(2)
    logits = torch.randn(B, C, generator=g) * 3
    labels = torch.randint(0, C, (B,), generator=g)
    soft = torch.rand(B, C, generator=g)
    return logits, labels, soft / soft.sum(-1, keepdim=True)


def _old_xent_metric(fault):
    """Worst (loss, dlogits) max|a-b| / max|b| of the faulty replay on the shapes and inputs of test_gpu_head.py (gradient
    scaled as there; the bars are 1e-6 and 1e-5)."""
    worst = [0.0, 0.0]
    for B, C in OLD_XENT_SHAPES:
        x, lab, soft = _old_xent_inputs(B, C)
        for t in (lab, soft):
            r = S.xent_f64(x, t, gloss=1.7)
            got = S.xent_replay32(x, t, gloss=1.7, **fault)
            worst = [max(worst[0], relerr(got['mean'], r['mean'])), max(worst[1], relerr(got['dx'], r['dx']))]
    return worst


def _structure_rejects(c, got):
    return sum(int(X.mismatch(got[k].reshape(c[k].shape), c[k]).sum()) for k in ('rows', 'mean', 'dx', 'lse'))


def test_xent_faults_rejected():
    """Rows >= 256 left out of the mean, the last lane-tail columns skipped, the lse offset error: what the tolerance test
    measures for each on its shapes, and that the new cases reject it."""
    # rows >= 256: the old shapes have at most 64 rows, the fault is not reachable
    e = _old_xent_metric(dict(rows_limit=256))
    assert e[0] <= 1e-6 and e[1] <= 1e-5
    c = S.xent_structure_case(257, 400, 'soft', seed=657)
    assert _structure_rejects(c, S.xent_replay32(c['x'], c['target'])) == 0, 'the replay itself passes'
    n = _structure_rejects(c, S.xent_replay32(c['x'], c['target'], rows_limit=256))
    report(f'ok   exact-sensitivity [xent] rows >= 256 left out of the mean: rejected ({n} elements); tolerance metric {e[0]:.1e} / '
           f'{e[1]:.1e} vs bars 1e-6 / 1e-5 (not reachable at B <= 64)')
    assert n > 0
    # the last trip of the lane loop skipped: the old test sees it on soft targets (reported), equality sees it on every shape with C > 64
    e = _old_xent_metric(dict(skip_tail=True))
    for B, C in ((5, 65), (7, 174), (1030, 1000)):
        c = S.xent_structure_case(B, C, 'soft', seed=B + C)
        n = _structure_rejects(c, S.xent_replay32(c['x'], c['target'], skip_tail=True))
        assert n > 0, (B, C)
    report(f'ok   exact-sensitivity [xent] last lane-tail columns skipped in the soft-target sums: rejected; tolerance metric '
           f'{e[0]:.1e} / {e[1]:.1e} vs bars 1e-6 / 1e-5')
    # the offset error: passes the old bars on the old inputs, misses the bound at offsets 64 and 4096
    e = _old_xent_metric(dict(form='kernel'))
    assert e[0] <= 1e-6 and e[1] <= 1e-5, e
    for off, must_fail in ((0, False), (64, None), (4096, True)):
        ok_all, worst = True, 0.0
        for tgt in ('labels', 'soft', 'smoothed'):
            c = S.xent_accuracy_case(257, 400, 3, off, tgt, seed=1)
            need, ok = S.xent_check(c['name'], S.xent_replay32(c['x'], c['target'], form='kernel'),
                                    S.xent_f64(c['x'], c['target']), S.K_GPU, quiet=True)
            ok_all, worst = ok_all and ok, max(worst, *need.values())
        report(f'ok   exact-sensitivity [xent] lse = mx + log(se) form at offset {off}: needs k = {worst:.1f} '
               f'({"passes" if ok_all else "rejected"} at K_GPU = {S.K_GPU}); tolerance metric on the old inputs {e[0]:.1e} / {e[1]:.1e}')
        if must_fail is not None:
            assert ok_all != must_fail


# --------------------------------------------------------------------------------------------------- top-k
def test_topk_reference_and_tie_rule():
    """On tie-free rows the reference equals torch.topk; on the tie cases the opposite tie rule gives another count for every
    shape with more than one column (the old test allows abs(diff) <= number of tied rows, which passes it)."""
    for B, C in S.XENT_SHAPES:
        s, lab = S.topk_free_case(B, C, seed=B + C)
        for k in S.topk_ks(C):
            want = int((s.topk(min(k, C), dim=-1).indices == lab[:, None]).any(-1).sum())
            assert S.topk_ref(s, lab, k) == want
        differs = 0
        for k in S.topk_ks(C):
            s, lab = S.topk_tie_case(B, C, k, seed=B + C + k)
            differs += S.topk_ref(s, lab, k) != S.topk_ref(s, lab, k, smaller_index_first=False)
        assert differs or C <= 2 or B < 2, (B, C)
    # the old test's inputs and its acceptance rule
    g = torch.Generator().manual_seed(3)
    scores = torch.randn(97, 50, generator=g)
    scores[:, 10] = scores[:, 11]
    labels = torch.randint(0, 50, (97,), generator=g)
    tied = int(sum(1 for r in range(97) if (scores[r] == scores[r, labels[r]]).sum() > 1))
    old_passes = all(abs(S.topk_ref(scores, labels, k, smaller_index_first=False) - S.topk_ref(scores, labels, k)) <= tied for k in (1, 5))
    s, lab = S.topk_tie_case(257, 400, 5, seed=662)
    a, b = S.topk_ref(s, lab, 5), S.topk_ref(s, lab, 5, smaller_index_first=False)
    report(f'ok   exact-sensitivity [topk] ties broken by the larger index: rejected ({b} for {a} rows correct at 257x400, k = 5); '
           f'the old rule abs(diff) <= {tied} tied rows {"passes" if old_passes else "rejects"} it')
    assert old_passes and a != b


# ------------------------------------------------------------------------------------------------ optimizer
@functools.lru_cache(maxsize=None)
def _lay():
    return S.MtLayout()


def test_layout_reaches_every_path():
    lay = _lay()
    assert 290 <= lay.n <= 310 and lay.numel < 2 ** 20 and lay.sizes[lay.n // 2] == 0
    assert all(len(ts) >= 1 for ts in lay.scalar_forced_by()), 'each pointer alone forces the scalar path of a full chunk'
    mis = (lay.off != 0).any(1).mean()
    assert 0.25 < mis < 0.42
    assert any(lay.sizes[t] >= S.MT_CHUNK and not lay.off[t].any() for t in range(lay.n)), 'the vector path runs too'
    for j in range(4):
        idx = lay.index[j]
        assert idx.unique().numel() == idx.numel() and int(idx.min()) >= S.GUARD and int(idx.max()) < lay.total[j] - S.GUARD


def test_norm_premises():
    lay = _lay()
    for kind in ('ints', 'clip'):
        norms, sq = S.mt_norms_expected(lay, S.mt_grads(lay, kind))
        pow2 = [float(n) for n in norms[:-1] if n >= 32 and math.log2(float(n)) % 1 == 0]
        if kind == 'clip':
            assert 64.0 in pow2 and 32.0 in pow2
            c = S.clip_coef(norms[:-1], 1.0)
            assert set(c.tolist()) == {2.0 ** -6, 2.0 ** -5, 1.0}, 'coef exactly 2^-6, 2^-5 or no clipping'
    one = torch.tensor(1e-6, dtype=F32)
    assert torch.tensor(32.0) + one == 32.0 and torch.tensor(16.0) + one != 16.0
    # tensors >= 256 missing from the norm of norms: not reachable with the 8 tensors of the old test
    norms, sq = S.mt_norms_expected(lay, S.mt_grads(lay, 'ints'))
    bad = sq[:256].sum().sqrt().float()
    report(f'ok   exact-sensitivity [optim] tensors >= 256 missing from the norm of norms: rejected ({float(bad):.6g} for '
           f'{float(norms[-1]):.6g}); not reachable with the {len(OLD_OPT_SHAPES)} tensors of the tolerance test')
    assert bad != norms[-1]


def test_sgd_exact_premise_and_chunk_fault():
    lay = _lay()
    for clip in (0.0, 1.0):
        for nesterov in (True, False):
            res = S.sgd_exact_expected(lay, clip, nesterov, False)
            res1 = S.sgd_exact_expected(lay, clip, nesterov, True)
            assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(res, res1)), 'first_step from a zero buffer'
    # a scalar-path chunk processed twice: the first full chunk of a tensor whose p pointer is misaligned
    t = lay.scalar_forced_by()[0][0]
    p0, g, lr, wd = S.mt_params(lay), S.mt_grads(lay, 'ints'), *lay.hyper(S.MT_GROUPS)
    p1, m1 = S.sgd_step(p0, g, torch.zeros_like(p0), 1.0, lr, wd, 0.5, True, False)
    sel = (lay.tid == t).nonzero()[:S.MT_CHUNK, 0]
    p2, _ = S.sgd_step(p1[sel], g[sel], m1[sel], 1.0, lr[sel], wd[sel], 0.5, True, False)
    n = int((p2 != p1[sel]).sum())
    report(f'ok   exact-sensitivity [optim] a scalar-path chunk of a misaligned tensor processed twice: rejected ({n} of {len(sel)} '
           f'elements differ); the tolerance test has no misaligned tensor')
    assert n > 0


def test_adamw_exact_premise():
    lay = _lay()
    for wd_on in (False, True):
        for preload in (False, True):
            r = S.adamw_exact_case(lay, wd_on, preload)
            X.assert_fp32_exact('p', r['p'])
            assert bool((r['p'] != r['p0']).any()) and bool((r['q'] != 0).any())


@functools.lru_cache(maxsize=None)
def _general_k(kind):
    """K of the float32 transcription of four general steps (state carried in float32), per output."""
    lay = _lay()
    groups = [list(gp) for gp in S.MT_GROUPS_GENERAL[kind]]
    p = S.general_data(lay, kind, -1)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    worst = {}
    for step in range(4):
        if step == 2:
            groups[1][1] = 0.02
            groups[0][0] *= 0.5
        lr, wd = lay.hyper(groups)
        g = S.general_data(lay, kind, step)
        sq = torch.zeros(lay.n, dtype=F64).index_add_(0, lay.tid, g * g)
        c = 0.5 / (sq.sqrt().float().double() + 1e-6)
        coef = lay.per_element(torch.where(c < 1, c, torch.ones_like(c)))
        h = dict(mom=float(torch.tensor(0.9, dtype=F32))) if kind == 'sgd' else S.adamw_hyper(0.9, 0.999, 1e-8, step + 1)
        ref = S.general_step64(kind, p, g, m, v, coef, lr, wd, h)
        got = S.general_step32(kind, p, g, m, v, coef, lr, wd, h)
        for grp in (0, 1):
            sel = torch.tensor(lay.group)[lay.tid] == grp
            need, _ = S.opt_check(f'{kind} transcription step {step}', kind, got, ref, math.inf, quiet=True, sel=sel)
            worst[grp] = {k: max(x, worst.get(grp, {}).get(k, 0.0)) for k, x in need.items()}
        p, m = got['p'].double(), got['m'].double()
        v = got['v'].double() if kind == 'adamw' else v
    return worst


@pytest.mark.parametrize('kind', ['sgd', 'adamw'])
@pytest.mark.parametrize('grp', [0, 1])
def test_general_step_transcription_within_k(kind, grp):
    need = _general_k(kind)[grp]
    K = S.K_OPT[kind][grp]
    worst = max(need.values())
    report(f'ok   optimizer K [{kind}, {"decayed" if grp else "no-decay"} group]: the float32 transcription of four general steps needs ' +
           ', '.join(f'{k} K={v:.2f}' for k, v in need.items()) + f' (K = {K})')
    assert K / 2 < worst <= K, f'K = {K} is not the next power of two above {worst:.3f}'


def test_clip_without_the_1e_6_is_rejected():
    """coef = clip / n without the 1e-6: invisible to max|a-b| / max|b| <= 2e-6 on the tensors of the old test (norms in the
    hundreds), beyond the bound on the momentum of the small tensors whose norm is near the threshold."""
    lay = _lay()
    kind, clip = 'sgd', 0.5
    p, g = S.general_data(lay, kind, -1), S.general_data(lay, kind, 0)
    lr, wd = lay.hyper(S.MT_GROUPS_GENERAL[kind])
    n32 = torch.zeros(lay.n, dtype=F64).index_add_(0, lay.tid, g * g).sqrt().float().double()
    good, bad = clip / (n32 + 1e-6), clip / n32.clamp_min(1e-300)
    coefs = [lay.per_element(torch.where(c < 1, c, torch.ones_like(c))) for c in (good, bad)]
    h = dict(mom=float(torch.tensor(0.9, dtype=F32)))
    z = torch.zeros_like(p)
    ref = S.general_step64(kind, p, g, z, z, coefs[0], lr, wd, h)
    got = S.general_step32(kind, p, g, z, z, coefs[1], lr, wd, h)
    bar = 2 * S.K_OPT['sgd'][0]
    need, ok = S.opt_check('sgd clip without 1e-6', kind, got, ref, bar, quiet=True)
    old = max(relerr(got['p'][lay.tid == t], ref['p'][lay.tid == t]) for t in range(lay.n) if lay.sizes[t])
    report(f'ok   exact-sensitivity [optim] coef = clip / n without the 1e-6: rejected (m needs K = {need["m"]:.1f}, bar {bar}); '
           f'tolerance metric {old:.1e} vs bar 2e-6')
    assert not ok and old <= 2e-6


# ------------------------------------------------------------------------------------------------- MaskFeat
def test_maskfeat_premises_and_second_lane_trip():
    tok = S.mf_token(96)
    ties, inexact = X.bf16_stats(tok)
    X.expect_bf16('mask token', tok, 'round')
    report(f'ok   maskfeat mask token: {ties:.0%} ties and {inexact:.0%} inexact outputs under the bf16 store')
    one = torch.tensor(1e-5, dtype=F32)
    assert torch.tensor(255.0) + one != 255.0 and torch.tensor(256.0) + one == 256.0, 'where n + 1e-5f stops changing n'
    for Cf in (64, 128, 24, 108):
        c = S.mf_loss_case(1, 2, 2, 3, Cf, 5, F32, pad=8)
        e = (c['diff'] * c['diff']).sum(1)
        assert float(e.max()) * 64 < 2 ** 53 and torch.equal((e * 64).round(), e * 64)
        if c['exact']:
            assert torch.equal((e / Cf) * Cf, e)
    # the second trip of the lane loop over Cf dropped: not reachable at Cf = 24
    old = S.mf_loss_case(2, 4, 2, 3, 24, 20, F32)
    assert old['Cf'] <= 64
    c = S.mf_loss_case(1, 2, 2, 3, 128, 5, F32)
    e1 = (c['diff'][:, :64] ** 2).sum(1)
    bad = (e1 / 128 * c['cmask']).sum()
    report(f'ok   exact-sensitivity [maskfeat] the second lane trip over Cf dropped: rejected ({float(bad):.6g} for {float(c["lsum"]):.6g}); '
           f'not reachable at Cf = 24')
    assert bad != c['lsum']
