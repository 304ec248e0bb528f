"""CPU checks of the exact-arithmetic test machinery (tests/exact.py): the premise of every case table that
test_gpu_exact_arith.py uses, the bf16 rounding table, and that check_exact rejects the kernel faults a float64
tolerance check lets through (emulated on the CPU: float64 -> float32 -> RNE bf16, the same arithmetic as the kernels)."""
import pytest
import torch

import exact as X
from helpers import relerr, report

BF16_BAR = 1e-2          # the tolerance test_gpu_kernels.py holds bf16 GEMM outputs to


def test_rne_table():
    v = torch.tensor([257., 259., 261., 514., 513., 515., 518., 1028., 1030., 0.5 + 2 ** -9, 1 + 2 ** -8, 1 + 3 * 2 ** -8])
    want = torch.tensor([256., 260., 260., 512., 512., 516., 520., 1024., 1032., 0.5, 1., 1 + 2 ** -6])
    for sign in (1, -1):
        got = X.rne_bf16((sign * v).double()).double()
        assert torch.equal(got, (sign * want).double()), (sign, got)
    ties, inexact = X.bf16_stats(torch.tensor([256., 257., 258., 259., 512., 514., 515., -514.]).double())
    assert (ties, inexact) == (4 / 8, 5 / 8)       # ties 257, 259, 514, -514; inexact besides: 515
    with pytest.raises(AssertionError):
        X.assert_fp32_exact('2^24 + 1', torch.tensor([2.0 ** 24 + 1], dtype=torch.float64))
    with pytest.raises(AssertionError):
        X.assert_fp32_exact('2^24', torch.tensor([2.0 ** 24], dtype=torch.float64))
    with pytest.raises(AssertionError):
        X.expect_bf16('257', torch.tensor([257.], dtype=torch.float64), 'exact')


def test_case_premises():
    """Every case the GPU file builds satisfies its premise (the builders assert it: accumulator bound < 2^24, every
    epilogue intermediate fp32-exact, exact-range outputs representable, rounding outputs >= 20 % ties, >= 40 % inexact)."""
    for M, N, K, kind in X.NT_SHAPES + X.NT_NODMA_SHAPES:
        A, W, b = X.nt_operands(M, N, K, kind, seed=M)
        X.expect_bf16(f'{M}x{N}x{K}', X.nt_reference('shape', A, W, bias=b), kind)
    for i, epi in enumerate(X.NT_EPILOGUES):
        for kind in ('exact', 'round'):
            if epi == 'plain' and kind == 'round':
                continue
            c = X.nt_epilogue_case(epi, kind, seed=10 * i)
            for key in ('expected', 'expected_split', 'expected_pre'):
                if key in c:
                    X.expect_bf16(f'{epi} {kind} {key}', c[key], kind)
    A, B = X.tn_operands(6000, 768, 512)
    X.tn_reference('tn', A, B)


def _trunc_bf16(v):
    """The faulty store: bf16 by truncation of the fp32 pattern."""
    return (v.float().view(torch.int32) & ~0xFFFF).view(torch.float32).to(torch.bfloat16)


def _faults(c):
    """(name, faulty float64 result) for one flat epilogue case: the kernel bugs that keep every value plausible."""
    A, W = c['A'].double(), c['W'].double()
    bias = c['bias'].double() if c['bias'] is not None else 0.0
    s = c['scale'].double().repeat_interleave(X.TOK_T)[:, None] if c['scale'] is not None else 1.0
    good = c['expected']
    out = []
    # one K term dropped in one output column: the term with the most non-zero products
    n = 5
    k = int((A != 0).double().mul(W[n] != 0).sum(0).argmax())
    bad = good.clone()
    bad[:, n] -= A[:, k] * W[n, k] * (s[:, 0] if torch.is_tensor(s) else s)
    out.append(('dropped K term', bad))
    # one row read through the neighbouring row-map group (token row of the next clip)
    bad = good.clone()
    m = 3
    bad[m] = ((A[m + X.TOK_N] @ W.t()) + bias) * (s[m] if torch.is_tensor(s) else s)
    out.append(('neighbouring group row', bad))
    # one row takes the row scale of the neighbouring row group
    if torch.is_tensor(s):
        g = int((c['scale'][1:] != c['scale'][:-1]).nonzero()[0])          # a group whose neighbour has another scale
        rows = slice(g * X.TOK_T, (g + 1) * X.TOK_T)
        bad = good.clone()
        bad[rows] = (A[rows] @ W.t() + bias) * c['scale'][g + 1].double()
        out.append(('neighbouring row scale', bad))
    # one 64-deep K tile summed twice
    bad = good + (A[:, 64:128] @ W[:, 64:128].t()) * s
    out.append(('K tile summed twice', bad))
    return out


@pytest.mark.parametrize('kind', ['exact', 'round'])
def test_check_exact_rejects_faults(kind):
    """Every injected fault is rejected by the exact comparison, on both generators; the float64 tolerance metric of each
    is reported next to the bf16 bar (not asserted: it is the gap these tests close)."""
    c = X.nt_epilogue_case('scale', kind, K=192)
    want = X.expect_bf16('scale', c['expected'], kind)
    assert not X.mismatch(X.rne_bf16(c['expected']), want).any()
    for name, bad in _faults(c):
        got = X.rne_bf16(bad)
        nbad = int(X.mismatch(got, want).sum())
        e = relerr(got.double(), c['expected'])
        report(f'ok   exact-sensitivity [{kind}] {name}: rejected ({nbad} elements differ); '
               f'tolerance metric {e:.2e} vs bf16 bar {BF16_BAR:g}')
        assert nbad > 0, f'{kind}: fault "{name}" passes the exact comparison'
    got = _trunc_bf16(c['expected'])
    nbad = int(X.mismatch(got, want).sum())
    e = relerr(got.double(), c['expected'])
    if kind == 'round':
        report(f'ok   exact-sensitivity [{kind}] truncating store: rejected ({nbad} elements differ); '
               f'tolerance metric {e:.2e} vs bf16 bar {BF16_BAR:g}')
        assert nbad > 0
    else:
        # exact-range outputs are representable: truncation and RNE agree on them by construction -- the rounding
        # cases exist for this fault
        assert nbad == 0


def test_check_exact_sentinels(monkeypatch):
    monkeypatch.setattr(X, 'report', lambda line: None)      # the self-test's deliberate failures stay out of the report
    buf = X.guarded((4, 16), torch.bfloat16, 'cpu')
    buf[:, :16] = 1.0
    X.check_exact('sentinel self-test', buf[:, :16], torch.ones(4, 16, dtype=torch.bfloat16), [buf[:, 16:]])
    buf[2, 17] = 0.0                                    # a stray store beyond N
    with pytest.raises(AssertionError, match='guard elements'):
        X.check_exact('sentinel self-test', buf[:, :16], torch.ones(4, 16, dtype=torch.bfloat16),
                      [buf[:, 16:]])
    with pytest.raises(AssertionError, match='1 of 64 elements differ'):
        want = torch.ones(4, 16, dtype=torch.bfloat16)
        want[1, 3] = 2
        X.check_exact('mismatch self-test', buf[:, :16], want)
