"""CPU checks of the table row-map test machinery (tests/exact_tab.py): the premises of every layout and case that
test_gpu_exact_rowmap_table.py runs -- the tables are the ones _compaction_plan builds, no kernel can mistake them for a closed
form (except the documented degenerate ones), a kernel that does stays inside the buffers, group boundaries fall where the group
sizes are meant to put them, and every expected value is fp32-exact (bf16 stores: rounding cases)."""
import pytest
import torch

import exact as X
import exact_ln as L
import exact_tab as T


def _both(lay):
    return (lay, lay.dropped())


@pytest.mark.parametrize('grp', T.GROUPS)
def test_tables_and_maps(grp):
    for kept in T.KEPT:
        lay = T.layout(grp, kept, T.base_of(grp, kept))
        for t in _both(lay):
            # the table of _compaction_plan: (clip index - group) * grp, the spare entry equal to the last; non-decreasing
            assert t.tab[:-1] == [(c - j) * grp for j, c in enumerate(t.kept)] and t.tab[-1] == t.tab[-2]
            assert all(b >= a for a, b in zip(t.tab, t.tab[1:]))
            assert t.max_step == max([b - a for a, b in zip(t.tab, t.tab[1:])] + [0])
            m = torch.arange(t.M)
            assert torch.equal(t.rows, t.base + m + torch.tensor(t.tab)[m // grp])
            # injective, inside the buffer, and exactly the rows of its clips
            assert t.rows.unique().numel() == t.M and int(t.rows.min()) >= t.base and int(t.rows.max()) < t.phys - T.TAIL
            clip_rows = torch.cat([t.base + c * grp + torch.arange(grp) for c in t.kept])
            assert torch.equal(t.rows, clip_rows)
            # the buffer bound: the closed form (grp, skip = max_step, base) of the table stays inside the allocation
            assert t.phys - T.TAIL >= t.base + t.M + t.n_groups * t.max_step + 1
            assert int(t.closed_rows(t.max_step).max()) < t.phys - T.TAIL
            assert int(t.unmapped().sum()) == t.phys - t.M
        kept_l, drop_l = _both(lay)
        # the two maps partition the clips' rows
        both = torch.cat([kept_l.rows, drop_l.rows]).sort().values
        assert torch.equal(both, lay.base + torch.arange(T.N_UNITS * grp))
        assert kept_l.phys == drop_l.phys


def test_patterns():
    """What the fixed patterns are meant to exercise."""
    a, b, c, d = (T.table_of(k, 1) for k in T.KEPT)
    assert a == [0, 2, 2, 5, 5] and b == [2, 2, 5, 5] and c == [5, 5] and d == [0] * 9
    steps = [y - x for x, y in zip(a, a[1:])]
    assert steps[:3] == [2, 0, 3]


def _closed_form_skip(t):
    """The constant skip whose closed form (grp, skip, base) has the table's row set, or None: tab[j] == j * skip for every j."""
    if t.tab[0] != 0:
        return None
    if t.n_groups == 1:
        return 0
    s = t.tab[1]
    return s if all(t.tab[j] == j * s for j in range(t.n_groups)) else None


@pytest.mark.parametrize('grp', T.GROUPS)
def test_not_a_closed_form(grp):
    """The row set of every table differs from the closed form (grp, skip = max_step, base), from ignoring the table (skip = 0)
    and from the closed form with ANY constant skip -- except the documented degenerate kept patterns: the all-zero table IS the
    closed form with skip 0, and the single group has no step (its tab[0] != 0 still has to be added: it differs from every
    closed form over `base` as well)."""
    n_real = 0
    for kept in T.KEPT:
        lay = T.layout(grp, kept, T.base_of(grp, kept))
        for t in _both(lay):
            s = _closed_form_skip(t)
            if t.kept == T.DEGENERATE[1]:
                assert s == 0 and t.tab == [0] * (t.n_groups + 1)
                continue
            assert s is None, f'{t} is the closed form with skip {s}'
            cands = {0, t.max_step, t.tab[1], t.tab[-1]} | (set(range(0, t.tab[-1] + 2)) if grp < 64 else set())
            for skip in cands:
                assert not torch.equal(t.closed_rows(skip), t.rows), f'{t} is the closed form with skip {skip}'
            if t.n_groups == 1:
                assert t.kept == T.DEGENERATE[0] or t is not lay      # a single group: the kept pattern [5], the complement [8]
                continue
            assert len(set(b - a for a, b in zip(t.tab[:-1], t.tab[1:-1]))) > 1, 'several different steps'
            n_real += 1
    assert n_real == 5          # kept [0, 3, 4, 8] and [2, 3, 7], and the complements with more than one clip


def test_boundaries_inside_tiles_and_passes():
    """grp 257 and 300: some group boundary lies strictly inside a 256-row tile and strictly inside a 16-row pass; grp 256: none
    does; grp 44: several boundaries inside one tile."""
    for grp in T.GROUPS:
        for kept in T.KEPT:
            for t in _both(T.layout(grp, kept, T.base_of(grp, kept))):
                bnd = t.boundaries()
                in_tile = [b for b in bnd if b % 256 != 0]
                in_pass = [b for b in bnd if b % 16 != 0]
                if grp == 256:
                    assert not in_tile and not in_pass
                elif bnd:
                    assert in_tile and in_pass
                if grp == 44 and len(bnd) >= 2:
                    assert len([b for b in bnd if b < 256]) >= 2
                if grp >= 256:                       # at most one boundary per 256-row tile: what the fast tile map assumes
                    tiles = [b // 256 for b in in_tile]
                    assert len(tiles) == len(set(tiles))
    assert any(len(t.boundaries()) > 0 for kept in T.KEPT for t in _both(T.layout(257, kept, 1)))


def test_gemm_case_premises():
    """Every GEMM case: fp32-exact at every step of the epilogue (asserted by exact.nt_reference), bf16 outputs a rounding case,
    the residual buffers hold junk outside their map, and the two maps of the mixed cases address different rows."""
    for grp, kept, epi, K in T.gemm_cases():
        c = T.gemm_case(grp, kept, epi, K)
        name = f'tab gemm {epi} grp={grp} kept={list(kept)} K={K}'
        X.assert_fp32_exact(name, c['expected'])
        X.expect_bf16(name, c['expected'], c['kind'])
        assert c['expected'].shape == (c['M'], c['N']) and c['M'] <= 2400
        if c['R'] is not None:
            assert bool((c['R'][c['rlay'].unmapped()] != 0).all())
            X.assert_fp32_exact(name + ' R', c['R'])
            assert torch.equal(X.rne_bf16(c['R'].double()).float(), c['R'])
        if epi in ('ctab_rclosed', 'cclosed_rtab'):
            assert c['rlay'] is not c['clay'] and not torch.equal(c['rlay'].rows, c['clay'].rows)
            closed = c['rlay'] if epi == 'ctab_rclosed' else c['clay']
            assert closed.rows.unique().numel() == c['M'] and int(closed.rows.max()) < closed.phys - T.TAIL
        if c['scale'] is not None:
            assert c['scale'].numel() == c['lay'].n_groups and bool((c['scale'] != 0).all())


def test_copy_case_premises():
    for grp in T.GROUPS:
        for kept in T.KEPT:
            c = T.copy_case(grp, kept)
            e = T.copy_expected(c)
            lay = c['lay']
            assert bool((c['src'] != 0).all())
            for k in ('gather', 'fix', 'colsum'):
                X.assert_fp32_exact(f'copy {k} {lay}', e[k])
                X.expect_bf16(f'copy {k} {lay}', e[k], 'exact') if k != 'colsum' else None
            assert torch.equal(X.rne_bf16(c['src'].double()).float(), c['src'])
            drop = e['drop']
            assert drop.numel() == lay.M and bool(drop[0]) and bool(drop[-1]) and not bool(drop.all())
            # partial sums of the column sums stay exact in any order
            L.assert_sums_exact(f'copy colsum {lay}', c['src'][lay.rows][drop], 0, 1.0)
            if grp == 257:
                assert lay.M % T.FIX_GROUP != 0 or lay.n_groups % 4 == 0


@pytest.mark.parametrize('grp', T.GROUPS)
def test_layernorm_case_premises(grp):
    """The exact_ln builders assert their own premises; the row counts are those of the table layouts."""
    for rows in T.ln_rows_of(grp):
        for D in T.LN_D + T.LN_D_WIDE:
            for kind in T.LN_FWD_KINDS + (T.LN_ACC_KINDS if D <= 1024 else ()):
                c = L.fwd_case(rows, D, kind, L.case_seed(rows, D))
                L.fwd_expected_y(c, c['rstd'].float())
                if kind in T.LN_ACC_KINDS:
                    assert torch.equal(X.rne_bf16(c['d'].double()).float(), c['d'])
        for D in T.LN_D:
            for kind in T.LN_BWD_KINDS:
                c = L.bwd_case(rows, D, kind, True, L.case_seed(rows, D))
                L.bwd_expected_dx(c)
                X.assert_fp32_exact(c['name'] + ' dgamma', c['dgamma'])
                X.assert_fp32_exact(c['name'] + ' dbeta', c['dbeta'])


def test_layout_carries_a_table():
    """exact_ln.Layout with a table places and gathers through the index vector; without one it is what it was."""
    tl = T.layout(257, T.KEPT[1], 4)
    lay = L.Layout(tl.M, table=tl)
    assert torch.equal(lay.idx, tl.rows) and lay.phys == tl.phys and (lay.n, lay.skip, lay.base) == (257, tl.max_step, 4)
    vals = X.ints((tl.M, 8), -4, 4, 1.0, 1)
    buf = lay.place(vals, pad=4)
    assert buf.shape == (tl.phys, 12) and torch.equal(lay.got(buf, 8), vals) and bool((buf[lay.unmapped] != 0).all())
    assert torch.equal(lay.unmapped, tl.unmapped())
    old = L.Layout(100)
    m = torch.arange(100)
    assert torch.equal(old.idx, 1 + m + m // L.TOK_N) and old.phys == int(old.idx[-1]) + 3 and old.table is None
    ident = L.Layout(50, n=50, skip=0, base=0)
    assert torch.equal(ident.idx, torch.arange(50))
